// mm_api.hip — the C ABI (include/simd_minimizers_amd.h): plan, workspace and run entry points.
//
// Mirrors the reference's builder (src/lib.rs:225-577): a plan is the immutable Builder
// {k, w, hasher, CANONICAL, SYNCMER}; a workspace is the reusable scratch the reference keeps
// in thread-locals (src/lib.rs:217-219, src/collect.rs:124-126), here device buffers + a stream.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <new>
#include <algorithm>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/simd_minimizers_amd.h"
#include "mm_env.h"
#include "mm_launch.h"
#include "mm_fasta_text.h"
#include "mm_lane_counts.h"
#include "mm_text_counts.h"
#include "mm_values_batch.h"
#include "mm_values_block.h"  // values_grid
#include "mm_one_min.h"
#include "mm_values_reads.h"
#include "mm_values_text.h"
#include "mm_bgzf.h"

namespace {

// Every exported function leaves the calling thread's CURRENT DEVICE as it found it (round 6): the entry
// points select their workspace's device - a device group's entries one after the other - and a caller that works with
// several devices must not find its own selection changed behind its back.  ApiScope marks an exported function's
// extent; set_device() notes the device the thread had when the outermost scope first changes it, the outermost scope's
// end puts it back.  (Threads the library starts itself - one per entry of the host-buffer group calls - have no scope and
// keep what they select until they end.)
struct ApiDeviceState {
    int depth = 0;
    int saved = -1;
    bool changed = false;
};
thread_local ApiDeviceState t_api_dev;
struct ApiScope {
    ApiScope() { ++t_api_dev.depth; }
    ~ApiScope() {
        if (--t_api_dev.depth == 0 && t_api_dev.changed) {
            (void)hipSetDevice(t_api_dev.saved);
            t_api_dev.changed = false;
        }
    }
    ApiScope(const ApiScope &) = delete;
    ApiScope &operator=(const ApiScope &) = delete;
};
hipError_t set_device(int device) {
    if (t_api_dev.depth > 0 && !t_api_dev.changed) {
        int cur = 0;
        if (hipGetDevice(&cur) == hipSuccess) {
            t_api_dev.saved = cur;
            t_api_dev.changed = true;
        } else {
            (void)hipGetLastError();
        }
    }
    return hipSetDevice(device);
}

thread_local std::string g_last_error;

int hip_fail(hipError_t e, const char *what) {
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
    return MM_ERR_HIP;
}
#define MM_HIP(call)                                   \
    do {                                               \
        hipError_t e_ = (call);                        \
        if (e_ != hipSuccess) return hip_fail(e_, #call); \
    } while (0)

uint32_t rotl32(uint32_t x, uint32_t r) {
    r &= 31u;
    return r ? (x << r) | (x >> (32u - r)) : x;
}
uint32_t rotr32(uint32_t x, uint32_t r) { return rotl32(x, 32u - (r & 31u)); }

// seq-hash 0.2.0 NtHasher (not in the reference tree): low halves of the classic ntHash
// seeds (values: bench/src/nthash.rs:24-32) indexed by the packed 2-bit code, 7 bits of
// rotation per base, complement = code ^ 2.  Pinned by the doctests src/lib.rs:92-140.
const uint32_t kNtSeeds[4] = {0x95c60474u, 0x62a02b4cu, 0x82572324u, 0x4be24456u};

mm::HashTables make_tables(const mm_hasher_t &h, uint32_t k) {
    mm::HashTables t;
    const uint32_t R = h.rot & 31u;
    uint32_t fw_out[4], rc_in[4], rc_out[4];
    for (int c = 0; c < 4; ++c) {
        fw_out[c] = rotl32(h.fw[c], (uint32_t)(((uint64_t)R * k) & 31u));
        rc_in[c] = rotl32(h.rc[c], (uint32_t)(((uint64_t)R * (k - 1)) & 31u));
        rc_out[c] = rotr32(h.rc[c], R);
    }
    for (int out = 0; out < 4; ++out)
        for (int in = 0; in < 4; ++in) {
            t.t_in_out[(out << 2) | in].x = h.fw[in] ^ fw_out[out];
            t.t_in_out[(out << 2) | in].y = rc_in[in] ^ rc_out[out];
        }
    for (int in = 0; in < 4; ++in) {
        t.t_in[in].x = h.fw[in];
        t.t_in[in].y = rc_in[in];
    }
    // two add-only steps folded into one look-up (warm-up of a lane's first k-mer)
    for (int b = 0; b < 4; ++b)
        for (int a = 0; a < 4; ++a) {
            t.t_in2[(b << 2) | a].x = rotl32(t.t_in[a].x, R) ^ t.t_in[b].x;
            t.t_in2[(b << 2) | a].y = rotr32(t.t_in[a].y, R) ^ t.t_in[b].y;
        }
    // constant XOR terms of the hasher (0 for NtHasher): with g = state ^ C, one step maps
    // g -> rot(g) ^ T ^ rot(C) ^ C, so every table entry carries D = rot(C) ^ C (two-step entries
    // rot(D) ^ D) and the walk starts from C instead of 0 - nothing to do per base
    const uint32_t df = rotl32(h.fw_xor, R) ^ h.fw_xor, dr = rotr32(h.rc_xor, R) ^ h.rc_xor;
    for (int i = 0; i < 16; ++i) {
        t.t_in_out[i].x ^= df;
        t.t_in_out[i].y ^= dr;
        t.t_in2[i].x ^= rotl32(df, R) ^ df;
        t.t_in2[i].y ^= rotr32(dr, R) ^ dr;
    }
    for (int i = 0; i < 4; ++i) {
        t.t_in[i].x ^= df;
        t.t_in[i].y ^= dr;
    }
    t.fw0 = h.fw_xor;
    t.rc0 = h.rc_xor;
    t.rot = R;
    t.canonical = h.canonical ? 1u : 0u;
    return t;
}

// The rolling tables of a text hasher for one k (TextTables, mm_launch.h): make_tables' algebra with the (out, in) pair
// split into two look-ups, the constant XOR terms folded into t_in.
mm::TextTables make_text_tables(const mm_text_hasher_t &h, uint32_t k) {
    mm::TextTables t;
    const uint32_t R = h.rot & 31u;
    const uint32_t df = rotl32(h.fw_xor, R) ^ h.fw_xor, dr = rotr32(h.rc_xor, R) ^ h.rc_xor;
    for (int c = 0; c < 256; ++c) {
        t.t_in[c].x = h.fw[c] ^ df;
        t.t_in[c].y = rotl32(h.rc[c], (uint32_t)(((uint64_t)R * (k - 1)) & 31u)) ^ dr;
        t.t_out[c].x = rotl32(h.fw[c], (uint32_t)(((uint64_t)R * k) & 31u));
        t.t_out[c].y = rotr32(h.rc[c], R);
    }
    t.fw0 = h.fw_xor;
    t.rc0 = h.rc_xor;
    t.rot = R;
    t.canonical = h.canonical ? 1u : 0u;
    return t;
}

}  // namespace

struct mm_plan {
    uint32_t k, w;
    int canonical_windows;
    uint32_t mode;
    mm_hasher_t hasher;
    mm::HashTables ht;
    // text plans (mm_plan_create_text): byte input, 256-entry tables; hasher / ht above are unused
    bool text = false;
    mm::TextTables tt;
};

struct mm_workspace {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // scan state
    unsigned long long *status = nullptr;
    uint64_t status_words = 0;
    uint32_t *ticket = nullptr;
    unsigned long long *total = nullptr;    // [0] running total, [1] low word = error flag of the last run,
                                            // [2] low word = sticky error flag (mm_workspace_check)
    unsigned long long *h_total = nullptr;  // page-locked host copy of the words: [0] total, [1] error, [2] sticky
    unsigned long long *h_total_dev = nullptr;  // the same words as the device addresses them: the fused kernel's last
                                                // tile stores the run's total to [0], flag_error the code to [1]
    // look-back status words of the fused family carry the epoch of their launch (kEpochShift, mm_common.h)
    uint32_t status_epoch = 0;    // epoch of the last tagged launch
    bool status_dirty = true;     // the buffer may hold words that are not tagged (fresh allocation, generic family)
    bool force_ticket = false;
    bool async_unchecked = false;  // an *_async run was issued since the last mm_workspace_check
    // split path (walk + expander on a second stream): dump slots, tile status, redo list, fork / join events
    mm::SplitBuffers split;
    bool no_split = false;  // the split path failed once on this workspace: fused kernel from then on
    bool fasta_three_pass = false;  // a look-back of the one-pass FASTA packer timed out: three-pass kernels from then on
    bool fasta_three_once = false;  // this text has too many short lines for the one-pass packer's tables
    // diagnostics: shader-clock probe on a stream of its own (mm_clock_probe_*)
    hipStream_t probe_stream = nullptr;
    unsigned long long *probe_out = nullptr;
    // generic-path scratch
    void *scratch = nullptr;
    uint64_t scratch_bytes = 0;
    // staging for the host entry points
    void *d_in = nullptr;
    uint64_t d_in_bytes = 0;
    void *d_ascii = nullptr;
    uint64_t d_ascii_bytes = 0;
    uint32_t *d_out = nullptr;
    uint64_t d_out_elems = 0;
    uint32_t *d_sk = nullptr;
    uint64_t d_sk_elems = 0;
    // skip-ambiguous path: window ambiguity bits, staged ambiguity bits of the host entry points
    uint32_t *wamb = nullptr;
    uint64_t wamb_dwords = 0;
    // pipelined host entry point: copy streams, per-chunk events and pinned running totals
    hipStream_t copy_in = nullptr, copy_out = nullptr;
    hipEvent_t ev_in[64] = {}, ev_k[64] = {}, ev_out[64] = {};
    unsigned long long *h_pipe = nullptr;      // [64] page-locked: chunk c's kernel stores its running total here
    unsigned long long *h_pipe_dev = nullptr;  // the same words as the device addresses them
    unsigned long long *d_pipe = nullptr;      // [65] device: [0] = 0, [c + 1] = running total after chunk c (blit mode)
    // batch mode tables (sequence descriptors, tile -> sequence, per-sequence offsets)
    mm::BatchSeq *batch_seqs = nullptr;
    uint64_t batch_seqs_n = 0;
    mm::BatchTile *batch_tiles = nullptr;
    uint64_t batch_tiles_n = 0;
    unsigned long long *batch_offsets = nullptr;
    uint64_t batch_offsets_n = 0;
    unsigned long long *h_batch = nullptr;  // page-locked landing buffer of a batch launch's offsets
    // lane-table launches (round 6; mm_lanes.hip): the table, the tiles' origins, first lane per read, block sums, and -
    // batches of sequences - the uploaded starts and lengths
    mm::LaneSeg *seg_table = nullptr;
    uint64_t seg_table_n = 0;
    uint32_t *seg_origin = nullptr;
    uint64_t seg_origin_n = 0;
    uint32_t *seg_first = nullptr;
    uint64_t seg_first_n = 0;
    uint32_t *seg_blk = nullptr;
    uint64_t seg_blk_n = 0;
    unsigned long long *seg_starts = nullptr;
    uint64_t seg_starts_n = 0;
    uint32_t *seg_lens = nullptr;
    uint64_t seg_lens_n = 0;
    bool last_lane_table = false;  // the last reads / batch run was a lane-table launch (diagnostics)
    uint64_t last_lanes = 0;       // ... and the lanes of its (padded) table
    uint8_t *h_small = nullptr;             // page-locked staging of short host calls (run_host_small): bytes in, positions, indices
    uint8_t *h_small_dev = nullptr;         // ... as the device addresses it
    uint64_t h_batch_n = 0;
    void *d_amb = nullptr;
    uint64_t d_amb_bytes = 0;
    unsigned long long *d_vals = nullptr;
    uint64_t d_vals_elems = 0;
    // one minimizer per record (mm_one_minimizer_*): one 64-bit key per record
    unsigned long long *d_one_min_keys = nullptr;
    uint64_t d_one_min_keys_elems = 0;
    // text runs: a ring of device copies of text plans' tables, staged through page-locked slots; a slot is rewritten only
    // after the event of its last upload (kTextTableSlots - 1 other uploads later), so no text call waits for the stream
    static const int kTextTableSlots = 8;
    mm::TextTables *d_text_tables = nullptr;  // [kTextTableSlots]
    mm::TextTables *h_text_tables = nullptr;  // [kTextTableSlots] page-locked: what each device slot holds
    hipEvent_t ev_text_tables[kTextTableSlots] = {};
    bool text_slot_used[kTextTableSlots] = {};
    int text_slot_next = 0;
    // text batches (mm_run_text_batch_*): per tile, the range of record starts its collect stage reads
    unsigned long long *d_text_tiles = nullptr;
    uint64_t d_text_tiles_elems = 0;
    // batch values (mm_values_*_batch_device_async): the device tables - [n_seqs + 1 offsets | n_seqs descriptors] - and
    // two page-locked staging areas used in turn; an area is rewritten only after the event of its last upload
    uint8_t *d_vbatch = nullptr;
    uint64_t d_vbatch_bytes = 0;
    static const int kValuesBatchSlots = 2;
    uint8_t *h_vbatch[kValuesBatchSlots] = {};
    uint64_t h_vbatch_bytes[kValuesBatchSlots] = {};
    hipEvent_t ev_vbatch[kValuesBatchSlots] = {};
    bool vbatch_slot_used[kValuesBatchSlots] = {};
    int vbatch_slot_next = 0;
    // knobs / diagnostics
    bool force_generic = false;
    uint32_t nblk = 0;
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    double total_ms = 0.0;
    uint64_t launches = 0;
    int last_path = 0;
};

namespace {

template <class T>
int grow(T *&ptr, uint64_t &have, uint64_t need, size_t elem) {
    if (need <= have && ptr) return MM_OK;
    if (ptr) MM_HIP(hipFree(ptr));
    ptr = nullptr;
    have = 0;
    uint64_t want = need + need / 8 + 64;
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, want * elem);
    if (e != hipSuccess) {
        g_last_error = std::string("hipMalloc: ") + hipGetErrorString(e);
        return MM_ERR_ALLOC;
    }
    ptr = reinterpret_cast<T *>(p);
    have = want;
    return MM_OK;
}

// The workspace's byte buffers (d_in, d_amb, d_ascii, scratch) are void *: grow() for them.
int grow_bytes(void *&ptr, uint64_t &have, uint64_t need) {
    uint8_t *p = static_cast<uint8_t *>(ptr);
    const int r = grow(p, have, need, 1);
    ptr = p;
    return r;
}

// The first check of every DNA entry point: a text plan runs through mm_run_text_* only.
inline int dna_plan_only(const mm_plan_t *plan) { return plan && plan->text ? MM_ERR_BAD_MODE : MM_OK; }

// The tile status words.  MM_STATUS_TIGHT=1 (tests) allocates exactly what the launcher asked for, without
// the slack of grow(), so that an under-sized request cannot hide behind it.
int grow_status(mm_workspace *ws, uint64_t need) {
    static const bool tight = getenv("MM_STATUS_TIGHT") != nullptr;
    if (!tight) {
        if (!(need <= ws->status_words && ws->status)) ws->status_dirty = true;  // a fresh allocation holds anything
        return grow(ws->status, ws->status_words, need, sizeof(unsigned long long));
    }
    if (ws->status && ws->status_words == need) return MM_OK;
    ws->status_dirty = true;
    if (ws->status) MM_HIP(hipFree(ws->status));
    ws->status = nullptr;
    ws->status_words = 0;
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, need * sizeof(unsigned long long));
    if (e != hipSuccess) {
        g_last_error = std::string("hipMalloc: ") + hipGetErrorString(e);
        return MM_ERR_ALLOC;
    }
    ws->status = reinterpret_cast<unsigned long long *>(p);
    ws->status_words = need;
    return MM_OK;
}

// Epoch for the next launch of the fused family on this workspace's status words (kEpochShift, mm_common.h): the
// kernel reads every word of another epoch as "not yet", so nothing is cleared between launches.  The buffer is
// cleared when it may hold untagged words (fresh allocation, the generic family used it) and when the epochs wrap.
int next_status_epoch(mm_workspace *ws, uint32_t *epoch) {
    if (ws->status_dirty || ws->status_epoch >= mm::kEpochMax) {
        if (ws->status)
            MM_HIP(hipMemsetAsync(ws->status, 0, ws->status_words * sizeof(unsigned long long), ws->stream));
        ws->status_dirty = false;
        ws->status_epoch = 0;
    }
    *epoch = ++ws->status_epoch;
    return MM_OK;
}

#ifdef MM_EXPERIMENTS
// Buffers, second stream and events of the split path, grown to what the run needs.  (The split path - walk kernel +
// expander, mm_split.hip - measured slower than the fused kernel in round 3 and is a cross-check since: round 5 moved it
// out of the shipped library, it exists in the EXPERIMENTS build only)
int prepare_split(mm_workspace *ws, uint64_t tiles, uint64_t dump_bytes) {
    mm::SplitBuffers &b = ws->split;
    if (!b.aux) {
        int lo = 0, hi = 0;
        MM_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
        MM_HIP(hipStreamCreateWithPriority(&b.aux, hipStreamNonBlocking, hi));
        MM_HIP(hipEventCreateWithFlags(&b.ev_fork, hipEventDisableTiming));
        MM_HIP(hipEventCreateWithFlags(&b.ev_join, hipEventDisableTiming));
        void *p = nullptr;
        MM_HIP(hipMalloc(&p, 64));
        b.redo_n = reinterpret_cast<uint32_t *>(p);
        b.carry = reinterpret_cast<unsigned long long *>(p) + 1;
    }
    int r = grow(b.dump, b.dump_bytes, dump_bytes, 1);
    if (r) return r;
    r = grow(b.tile_status, b.status_words, tiles, sizeof(unsigned long long));
    if (r) return r;
    uint8_t *rl = reinterpret_cast<uint8_t *>(b.redo_list);
    uint64_t have = b.redo_entries;
    r = grow(rl, have, tiles, 16);
    b.redo_list = rl;
    b.redo_entries = have;
    return r;
}
#endif

int make_view(const void *d_packed, uint64_t packed_bytes, uint64_t base_offset, uint64_t n_bases,
              mm::SeqView *v) {
    uintptr_t a = reinterpret_cast<uintptr_t>(d_packed);
    uint64_t byte_shift = a & 3u;
    uint64_t base0 = base_offset + 4 * byte_shift;
    uint64_t n_dwords = (byte_shift + packed_bytes + 3) / 4;
    if (n_dwords == 0 || n_dwords >= (1ull << 32)) return MM_ERR_LEN_TOO_LARGE;
    if ((base0 + n_bases + 15) / 16 > n_dwords) return MM_ERR_CAPACITY;
    if (base0 >= (1ull << 32)) return MM_ERR_LEN_TOO_LARGE;
    v->d = reinterpret_cast<const uint32_t *>(a - byte_shift);
    v->n_dwords = (uint32_t)n_dwords;
    v->base0 = (uint32_t)base0;
    v->n_bases = (uint32_t)n_bases;
    return MM_OK;
}

int collect_timing(mm_workspace *ws) {
    for (auto &ev : ws->events) {
        MM_HIP(hipEventSynchronize(ev.second));
        float ms = 0.f;
        MM_HIP(hipEventElapsedTime(&ms, ev.first, ev.second));
        ws->total_ms += ms;
        ws->launches += 1;
        hipEventDestroy(ev.first);
        hipEventDestroy(ev.second);
    }
    ws->events.clear();
    return MM_OK;
}

// The per-run error word of a finished run (h_total[1], see OutParams::error): 0 = fine, 1 = a look-back
// spin ran out (the caller redoes the run in ticket mode), anything else is a failed launch.
// Returns 0 (fine), 1 (redo in ticket mode) or a negative MM_ERR_* code.
// (kernel error 6: the counts of a text batch run, read on the device, lie beyond the bounds the caller gave)
const char *const kTextCountsRefused =
    "mm_run_text_batch_counts_device_async: d_counts exceed max_chars / max_records (the loader overflowed its tables?); "
    "count 0 and offsets[0] = 0 were written, nothing else";
// (kernel error 7: the counts of a packed reads run, read on the device, lie beyond the bounds the caller gave)
const char *const kLaneCountsRefused =
    "mm_run_packed_reads_counts_device_async: d_counts exceed max_bases / max_records (the packer overflowed its table or "
    "buffer?); count 0 and offsets of 0 were written, no position";
// (kernel error 8: the counts of a one-minimizer call, read on the device, lie beyond the bounds the caller gave)
const char *const kOneMinCountsRefused =
    "mm_one_minimizer_*_counts_device_async: d_counts exceed the symbol / record bounds (the loader overflowed its tables?); "
    "every output word is MM_NO_MINIMIZER";
int judge_run_error(mm_workspace *ws) {
    const uint32_t code = (uint32_t)ws->h_total[1];
    if (code == 0) return 0;
    // The synchronous caller learns of this error right here (it repeats the run or returns the code), so the
    // sticky word the kernel raised with it (flag_error) is not news for mm_workspace_check - unless an
    // asynchronous run that has not been checked yet may have raised it too (then the check reports it: at
    // worst valid work is repeated).
    if (!ws->async_unchecked) (void)hipMemsetAsync(ws->total + 2, 0, sizeof(unsigned long long), ws->stream);
    // (the device's copy of the per-run word: consumed with the host's, so that no entry point that reads it back -
    // the pipelined host path, the FASTA wrapper - ever meets a stale code.  ADVICE r4)
    (void)hipMemsetAsync(ws->total + 1, 0, sizeof(unsigned long long), ws->stream);
    if (code == 1u) {
        if (ws->last_path == MM_PATH_SPLIT && !ws->no_split) {
            // the expander gave up waiting for a tile of the walk: this workspace keeps to the fused kernel
            ws->no_split = true;
            return 1;
        }
        if (ws->force_ticket) {
            g_last_error = "look-back scan timed out in ticket mode";
            return MM_ERR_HIP;
        }
        ws->force_ticket = true;
        return 1;
    }
    if (code == 3u) {
        // the one-pass FASTA packer met a text whose lines are too short for its tables: the three-pass kernels take
        // over on this workspace; the caller repeats the calls since the last check (as for a look-back time-out)
        ws->fasta_three_pass = true;
        g_last_error = "mm_fasta_pack_device_async: lines too short for the one-pass packer; its output is invalid, "
                       "repeat the call (three-pass kernels from now on)";
        return MM_ERR_ORDER;
    }
    if (code == 6u) {
        g_last_error = kTextCountsRefused;
        return MM_ERR_CAPACITY;
    }
    if (code == 7u) {
        g_last_error = kLaneCountsRefused;
        return MM_ERR_CAPACITY;
    }
    char buf[128];
    snprintf(buf, sizeof(buf), code == 2u   ? "kernel error 2: dynamic LDS does not lie behind the static LDS"
                               : code == 4u ? "kernel error 4: a skip-ambiguous launch without its LDS landing area"
                               : code == 5u ? "kernel error 5: the reads need more lanes than total_bases allows for"
                                            : "kernel error 0x%x (bad batch table)", code);
    g_last_error = buf;
    return MM_ERR_HIP;
}

// The synchronous form of every run: `issue(&host_written)` queues one attempt; the words total[0..1] come to h_total
// (a 16-byte copy, unless the kernel stores them into the page-locked words itself: host_written), the stream is waited
// for and the error word judged.  A look-back spin that ran out (1: workgroups were not dispatched in index order)
// repeats the run once, with tile ids taken from an atomic ticket, which defines the order itself.
template <class Issue>
int run_sync(mm_workspace_t *ws, uint64_t capacity, bool wants_positions, uint64_t *out_count, Issue issue) {
    if (!ws) return MM_ERR_NULL;
    for (int attempt = 0; attempt < 2; ++attempt) {
        // (an *_async run that is still executing on this stream stores its error code into the same page-locked
        // word: let it finish before the words are reused for THIS run, or its error would be taken for ours - the
        // sticky word keeps it for mm_workspace_check.  ADVICE r4)
        if (ws->async_unchecked) MM_HIP(hipStreamSynchronize(ws->stream));
        bool host_written = false;
        const int r = issue(&host_written);
        if (r) return r;
        if (!host_written)
            MM_HIP(hipMemcpyAsync(ws->h_total, ws->total, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ws->stream));
        MM_HIP(hipStreamSynchronize(ws->stream));
        const int je = judge_run_error(ws);
        if (je < 0) return je;
        if (je == 0) break;
    }
    if (out_count) *out_count = ws->h_total[0];
    if (wants_positions && ws->h_total[0] > capacity) return MM_ERR_CAPACITY;
    return MM_OK;
}

// Staging of the host entry points' results: room in d_out / d_sk for `cap` positions (and indices), cap being what the
// caller's buffer takes of the `bound` positions a run can give (0 when no positions are asked for) ...
uint64_t capped(const void *out_pos, uint64_t capacity, uint64_t bound) {
    return out_pos ? (capacity < bound ? capacity : bound) : 0;
}
int stage_outputs(mm_workspace_t *ws, uint64_t cap, bool want_sk) {
    int r = grow(ws->d_out, ws->d_out_elems, cap ? cap : 1, sizeof(uint32_t));
    if (r == MM_OK && want_sk) r = grow(ws->d_sk, ws->d_sk_elems, cap ? cap : 1, sizeof(uint32_t));
    return r;
}

// ... and their way back: `n_offsets` offsets from d_vals (batches), `count` positions (and indices) if they were asked
// for, and one wait when anything was queued.
int download_positions(mm_workspace_t *ws, uint32_t *out_pos, uint32_t *out_sk, uint64_t count, uint64_t *out_offsets,
                       uint64_t n_offsets) {
    if (out_offsets)
        MM_HIP(hipMemcpyAsync(out_offsets, ws->d_vals, n_offsets * sizeof(uint64_t), hipMemcpyDeviceToHost, ws->stream));
    if (out_pos && count) {
        MM_HIP(hipMemcpyAsync(out_pos, ws->d_out, count * sizeof(uint32_t), hipMemcpyDeviceToHost, ws->stream));
        if (out_sk) MM_HIP(hipMemcpyAsync(out_sk, ws->d_sk, count * sizeof(uint32_t), hipMemcpyDeviceToHost, ws->stream));
    }
    if (out_offsets || (out_pos && count)) MM_HIP(hipStreamSynchronize(ws->stream));
    return MM_OK;
}

// ---- launch arguments.  mm::RunArgs / ReadsArgs / TextRunArgs are value-initialised where they are filled (`a{}`): a
// field that a site does not name is null / 0.  What they take from the plan and the workspace is written here, once.
template <class Args>
void set_plan(Args &a, const mm_plan_t *plan) {
    a.k = plan->k;
    a.w = plan->w;
    a.mode = plan->mode;
    a.canonical_windows = plan->canonical_windows;
}
// (packed plans: the hasher's tables travel in the arguments; byte text keeps its tables on the device, set_text_tables)
template <class Args>
void set_packed_plan(Args &a, const mm_plan_t *plan) {
    set_plan(a, plan);
    a.ht = plan->ht;
}
// The per-run error word (OutParams::error; judge_run_error reads its host copy).
uint32_t *error_word(mm_workspace_t *ws) { return reinterpret_cast<uint32_t *>(ws->total + 1); }
// The outputs of a run on this workspace: the caller's positions / indices / capacity, the workspace's total, ticket and
// error words.  (status, count_out and total_host are the launch's own business.)
mm::OutParams out_params(mm_workspace_t *ws, uint32_t *pos, uint32_t *sk, uint64_t cap) {
    mm::OutParams o{};
    o.pos = pos;
    o.sk = sk;
    o.cap = cap;
    o.total = ws->total;
    o.ticket = ws->ticket;
    o.error = error_word(ws);
    return o;
}
int use_ticket(const mm_workspace_t *ws) { return (ws->force_ticket || mm::mm_env("MM_FORCE_TICKET")) ? 1 : 0; }
// Positions per window that a plan's mode gives on random sequence (sizes of lists and of first result buffers).
double expected_density(const mm_plan_t *plan) {
    return plan->mode == MM_OPEN_SYNCMERS ? 1.0 / plan->w : (plan->mode == MM_CLOSED_SYNCMERS ? 2.0 / plan->w : 2.0 / (plan->w + 1.0));
}
// The stand-in for a plan that the mm_debug_* planners fill their arguments from (no hasher, no device).  `mode` 3:
// minimizers WITH super-k-mer indices - their 16-bit list entries bound the lanes; 4: minimizers over a PackedNSeq - the
// skip-ambiguous walk's landing area and lane rules.
mm_plan_t debug_plan(uint32_t k, uint32_t w, int canonical_windows, int mode) {
    mm_plan_t p{};
    p.k = k;
    p.w = w;
    p.canonical_windows = canonical_windows;
    p.mode = (mode == 3 || mode == 4) ? 0u : (uint32_t)mode;
    return p;
}

// ---- the timed launch.  arm() creates an event pair when the workspace times its launches (mm_workspace_enable_timing)
// and hands it to the launch's arguments; done() - the launch is queued - gives the pair to ws->events, where
// collect_timing finds and destroys it, and notes the path that ran.  Every other way out of the scope destroys what was
// created: a second hipEventCreate that failed, a launcher that has no kernel for the plan, a refused launch, an
// allocation that failed in between.  ws->events therefore only holds pairs that were recorded.
class TimedLaunch {
  public:
    explicit TimedLaunch(mm_workspace_t *ws) : ws_(ws) {}
    TimedLaunch(const TimedLaunch &) = delete;
    TimedLaunch &operator=(const TimedLaunch &) = delete;
    ~TimedLaunch() { drop(); }
    template <class Args>
    int arm(Args &a) {
        a.timing_start = a.timing_stop = nullptr;
        if (!ws_->timing) return MM_OK;
        MM_HIP(hipEventCreate(&e0_));
        MM_HIP(hipEventCreate(&e1_));
        a.timing_start = e0_;
        a.timing_stop = e1_;
        return MM_OK;
    }
    void done(int path) {
        if (e0_) ws_->events.emplace_back(e0_, e1_);
        e0_ = e1_ = nullptr;
        ws_->last_path = path;
    }
    void drop() {
        if (e0_) hipEventDestroy(e0_);
        if (e1_) hipEventDestroy(e1_);
        e0_ = e1_ = nullptr;
    }

  private:
    mm_workspace_t *ws_;
    hipEvent_t e0_ = nullptr, e1_ = nullptr;
};
// (call it while the TimedLaunch is alive: the runtime's last error is the launch's, not an event's)
int launch_failed() {
    g_last_error = std::string("kernel launch failed: ") + hipGetErrorString(hipGetLastError());
    return MM_ERR_HIP;
}

// The page-locked landing buffer of a batch's offsets (a pageable one would make the copy block).
int grow_h_batch(mm_workspace_t *ws, uint64_t n) {
    if (ws->h_batch_n >= n) return MM_OK;
    if (ws->h_batch) hipHostFree(ws->h_batch);
    ws->h_batch = nullptr;
    ws->h_batch_n = 0;
    const uint64_t want = n * 2;
    MM_HIP(hipHostMalloc(reinterpret_cast<void **>(&ws->h_batch), want * sizeof(unsigned long long), hipHostMallocDefault));
    ws->h_batch_n = want;
    return MM_OK;
}

// The epilogue of the synchronous counts runs (packed reads, text batch): `issue` queues the run; the two counts come
// back with the run's words (h_total[4..5]: one wait for all of them).  out[0] = positions, out[1..2] = the counts, on
// MM_OK and on MM_ERR_CAPACITY (the need, or the true counts beyond their bounds); zeros otherwise.
template <class Issue>
int run_counts_sync(mm_workspace_t *ws, const uint64_t *d_counts, uint64_t capacity, bool wants_positions, uint64_t *out,
                    Issue issue) {
    if (out) out[0] = out[1] = out[2] = 0;
    uint64_t count = 0;
    const int r = run_sync(ws, capacity, wants_positions, &count, [&](bool *) {
        const int q = issue();
        if (q) return q;
        MM_HIP(hipMemcpyAsync(ws->h_total + 4, d_counts, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, ws->stream));
        return (int)MM_OK;
    });
    if (out && (r == MM_OK || r == MM_ERR_CAPACITY)) {
        out[0] = count;
        out[1] = ws->h_total[4];
        out[2] = ws->h_total[5];
    }
    return r;
}

}  // namespace

extern "C" {

const char *mm_strerror(int code) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    switch (code) {
        case MM_OK: return "ok";
        case MM_ERR_W_ZERO: return "w must be > 0";
        case MM_ERR_W_TOO_LARGE: return "w must be < 2^15";
        case MM_ERR_LEN_TOO_LARGE: return "sequence must be shorter than 2^32 bases";
        case MM_ERR_EVEN_L: return "canonical windows need odd l = k + w - 1";
        case MM_ERR_HASHER_NOT_CANONICAL: return "canonical windows need a canonical hasher";
        case MM_ERR_OPEN_EVEN_W: return "open syncmers need odd w";
        case MM_ERR_K_ZERO: return "k must be > 0";
        case MM_ERR_CAPACITY: return "buffer too small";
        case MM_ERR_BAD_MODE: return "bad mode (or super-k-mers requested with syncmers)";
        case MM_ERR_NULL: return "null argument";
        case MM_ERR_VALUE_LEN: return "values_u64 needs 1 <= len <= 32";
        case MM_ERR_FORMAT: return "FASTQ text (first record starts with '@'): only FASTA is packed on the device";
        case MM_ERR_NO_DEVICE: return "no HIP device (this engine has no CPU fallback)";
        case MM_ERR_HIP: return "HIP call failed";
        case MM_ERR_ALLOC: return "device allocation failed";
        case MM_ERR_ORDER: return "look-back timed out in an asynchronous run (repeat it; ticket mode is now on)";
        case MM_ERR_UNSORTED: return "record starts must not decrease";
        default: return "unknown error";
    }
}

const char *mm_last_error(void) { return g_last_error.c_str(); }

int mm_device_count(void) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int mm_default_hasher(mm_hasher_t *out, int canonical) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!out) return MM_ERR_NULL;
    for (int c = 0; c < 4; ++c) {
        out->fw[c] = kNtSeeds[c];
        out->rc[c] = kNtSeeds[c ^ 2];
    }
    out->rot = 7;
    out->canonical = canonical ? 1u : 0u;
    out->fw_xor = out->rc_xor = 0;
    out->kind = MM_HASHER_NT;
    return MM_OK;
}

// PARITY UNPINNED (seq-hash 0.2.0 is not in the reference tree; no known-answer vector exists): the
// published idea - "multiplies each character value by a pseudo-random constant" (src/lib.rs:71-72) -
// in NtHasher's rolling rot-xor form; constant and character offset are this engine's.
int mm_mul_hasher(mm_hasher_t *out, int canonical) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!out) return MM_ERR_NULL;
    for (uint32_t c = 0; c < 4; ++c) {
        out->fw[c] = (c + 1u) * 0x9E3779B1u;
        out->rc[c] = ((c ^ 2u) + 1u) * 0x9E3779B1u;
    }
    out->rot = 7;
    out->canonical = canonical ? 1u : 0u;
    out->fw_xor = out->rc_xor = 0;
    out->kind = MM_HASHER_MUL;
    return MM_OK;
}

// PARITY UNPINNED: the k-mer read as a base-4 number, first base most significant and inverted
// (anti-lexicographic order), left-aligned in 32 bits; the reverse strand likewise.
int mm_antilex_hasher(mm_hasher_t *out, uint32_t k, int canonical) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!out) return MM_ERR_NULL;
    if (k == 0) return MM_ERR_K_ZERO;
    const uint32_t sh = (32u - ((2u * k) & 31u)) & 31u;
    for (uint32_t c = 0; c < 4; ++c) {
        out->fw[c] = rotl32(c, sh);
        out->rc[c] = rotl32(c ^ 2u, sh);
    }
    out->rot = 2;
    out->canonical = canonical ? 1u : 0u;
    out->fw_xor = out->rc_xor = 3u << 30;  // the first base of either strand's k-mer sits at bits 30..31
    out->kind = MM_HASHER_ANTILEX;
    return MM_OK;
}

int mm_plan_create(mm_plan_t **out, uint32_t k, uint32_t w, int canonical_windows, mm_mode_t mode,
                   const mm_hasher_t *hasher) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!out) return MM_ERR_NULL;
    *out = nullptr;
    if (k == 0) return MM_ERR_K_ZERO;
    if (w == 0) return MM_ERR_W_ZERO;
    if (w >= (1u << 15)) return MM_ERR_W_TOO_LARGE;
    if ((int)mode < 0 || (int)mode > 2) return MM_ERR_BAD_MODE;
    if (mode == MM_OPEN_SYNCMERS && w % 2 == 0) return MM_ERR_OPEN_EVEN_W;
    mm_hasher_t h;
    if (hasher) h = *hasher;
    else mm_default_hasher(&h, canonical_windows);
    if (canonical_windows) {
        if (!h.canonical) return MM_ERR_HASHER_NOT_CANONICAL;
        if (((uint64_t)k + w - 1) % 2 == 0) return MM_ERR_EVEN_L;
    }
    mm_plan *p = new (std::nothrow) mm_plan;
    if (!p) return MM_ERR_ALLOC;
    p->k = k;
    p->w = w;
    p->canonical_windows = canonical_windows ? 1 : 0;
    p->mode = (uint32_t)mode;
    p->hasher = h;
    p->ht = make_tables(h, k);
    *out = p;
    return MM_OK;
}

// PARITY UNPINNED, like mm_mul_hasher: "multiplies each character value by a pseudo-random constant"
// (src/lib.rs:71-72) over bytes, in NtHasher's rolling form; the constant and the complement are this engine's.
int mm_text_mul_hasher(mm_text_hasher_t *out, int canonical) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!out) return MM_ERR_NULL;
    for (uint32_t c = 0; c < 256; ++c) {
        uint32_t comp = c;
        switch (c) {
            case 'A': comp = 'T'; break;
            case 'T': comp = 'A'; break;
            case 'C': comp = 'G'; break;
            case 'G': comp = 'C'; break;
            case 'a': comp = 't'; break;
            case 't': comp = 'a'; break;
            case 'c': comp = 'g'; break;
            case 'g': comp = 'c'; break;
            default: break;
        }
        out->fw[c] = c * 0x9E3779B1u;
        out->rc[c] = comp * 0x9E3779B1u;
    }
    out->rot = 7;
    out->canonical = canonical ? 1u : 0u;
    out->fw_xor = out->rc_xor = 0;
    out->kind = MM_HASHER_MUL;
    return MM_OK;
}

// packed-seq AsciiSeq's code of a byte, (c >> 1) & 3 (src/lib.rs:92-98), as a table over all 256 bytes
int mm_text_hasher_from_dna(mm_text_hasher_t *out, const mm_hasher_t *h) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!out || !h) return MM_ERR_NULL;
    for (uint32_t c = 0; c < 256; ++c) {
        out->fw[c] = h->fw[(c >> 1) & 3u];
        out->rc[c] = h->rc[(c >> 1) & 3u];
    }
    out->rot = h->rot;
    out->canonical = h->canonical;
    out->fw_xor = h->fw_xor;
    out->rc_xor = h->rc_xor;
    out->kind = h->kind;
    return MM_OK;
}

int mm_plan_create_text(mm_plan_t **out, uint32_t k, uint32_t w, int canonical_windows, mm_mode_t mode,
                        const mm_text_hasher_t *hasher) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!out) return MM_ERR_NULL;
    *out = nullptr;
    // (the checks of mm_plan_create, in its order)
    if (k == 0) return MM_ERR_K_ZERO;
    if (w == 0) return MM_ERR_W_ZERO;
    if (w >= (1u << 15)) return MM_ERR_W_TOO_LARGE;
    if ((int)mode < 0 || (int)mode > 2) return MM_ERR_BAD_MODE;
    if (mode == MM_OPEN_SYNCMERS && w % 2 == 0) return MM_ERR_OPEN_EVEN_W;
    mm_text_hasher_t h;
    if (hasher) h = *hasher;
    else mm_text_mul_hasher(&h, canonical_windows);
    if (canonical_windows) {
        if (!h.canonical) return MM_ERR_HASHER_NOT_CANONICAL;
        if (((uint64_t)k + w - 1) % 2 == 0) return MM_ERR_EVEN_L;
    }
    mm_plan *p = new (std::nothrow) mm_plan;
    if (!p) return MM_ERR_ALLOC;
    p->k = k;
    p->w = w;
    p->canonical_windows = canonical_windows ? 1 : 0;
    p->mode = (uint32_t)mode;
    memset(&p->hasher, 0, sizeof(p->hasher));
    memset(&p->ht, 0, sizeof(p->ht));
    p->text = true;
    p->tt = make_text_tables(h, k);
    *out = p;
    return MM_OK;
}

void mm_plan_destroy(mm_plan_t *plan) { delete plan; }

uint32_t mm_plan_value_len(const mm_plan_t *plan) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!plan) return 0;
    return plan->mode == MM_MINIMIZERS ? plan->k : plan->k + plan->w - 1;
}

int mm_workspace_create(mm_workspace_t **out, int device, void *hip_stream) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!out) return MM_ERR_NULL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        g_last_error = "no HIP device visible";
        return MM_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= n) return MM_ERR_NO_DEVICE;
    MM_HIP(set_device(device));
    mm_workspace *ws = new (std::nothrow) mm_workspace;
    if (!ws) return MM_ERR_ALLOC;
    ws->device = device;
    if (hip_stream) {
        ws->stream = reinterpret_cast<hipStream_t>(hip_stream);
    } else {
        // a BLOCKING stream: it orders itself against the legacy null stream, so callers that
        // fill / copy buffers on the default stream (torch does) need no extra events
        hipError_t e = hipStreamCreateWithFlags(&ws->stream, hipStreamDefault);
        if (e != hipSuccess) {
            delete ws;
            return hip_fail(e, "hipStreamCreate");
        }
        ws->own_stream = true;
    }
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&ws->ticket), 64);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&ws->total), 64);
    if (e == hipSuccess) {
        // page-locked, mapped and coherent: the kernel's last tile stores the run's total there itself.  A runtime
        // that refuses the flags still gives a plain page-locked block: the entry points then copy the words as
        // rounds 1-3 did (h_total_dev stays null).
        e = hipHostMalloc(reinterpret_cast<void **>(&ws->h_total), 64, hipHostMallocMapped | hipHostMallocCoherent);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            ws->h_total = nullptr;
            e = hipHostMalloc(reinterpret_cast<void **>(&ws->h_total), 64, hipHostMallocDefault);
        }
    }
    if (e == hipSuccess) {
        memset(ws->h_total, 0, 64);
        void *dp = nullptr;
        if (hipHostGetDevicePointer(&dp, ws->h_total, 0) == hipSuccess) ws->h_total_dev = reinterpret_cast<unsigned long long *>(dp);
        else (void)hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemset(ws->total, 0, 64);  // [0] total, [1] per-run error, [2] sticky error
    if (e == hipSuccess && ws->h_total_dev) {
        // [3]: where the host keeps its copy of the error word (flag_error stores the code there as well)
        const unsigned long long host_err = (unsigned long long)reinterpret_cast<uintptr_t>(ws->h_total_dev + 1);
        e = hipMemcpy(ws->total + 3, &host_err, sizeof(host_err), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        mm_workspace_destroy(ws);
        return hip_fail(e, "workspace allocation");
    }
    *out = ws;
    return MM_OK;
}

void mm_workspace_destroy(mm_workspace_t *ws) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!ws) return;
    set_device(ws->device);
    if (ws->stream) hipStreamSynchronize(ws->stream);
    for (auto &ev : ws->events) {
        hipEventDestroy(ev.first);
        hipEventDestroy(ev.second);
    }
    if (ws->status) hipFree(ws->status);
    if (ws->split.dump) hipFree(ws->split.dump);
    if (ws->split.tile_status) hipFree(ws->split.tile_status);
    if (ws->split.redo_list) hipFree(ws->split.redo_list);
    if (ws->split.redo_n) hipFree(ws->split.redo_n);  // (redo_n and carry share one allocation)
    if (ws->split.ev_fork) hipEventDestroy(ws->split.ev_fork);
    if (ws->split.ev_join) hipEventDestroy(ws->split.ev_join);
    if (ws->split.aux) hipStreamDestroy(ws->split.aux);
    if (ws->probe_stream) {
        hipStreamSynchronize(ws->probe_stream);
        hipStreamDestroy(ws->probe_stream);
    }
    if (ws->probe_out) hipFree(ws->probe_out);
    if (ws->ticket) hipFree(ws->ticket);
    if (ws->total) hipFree(ws->total);
    if (ws->h_total) hipHostFree(ws->h_total);
    if (ws->scratch) hipFree(ws->scratch);
    if (ws->d_in) hipFree(ws->d_in);
    if (ws->d_ascii) hipFree(ws->d_ascii);
    if (ws->d_out) hipFree(ws->d_out);
    if (ws->d_sk) hipFree(ws->d_sk);
    if (ws->wamb) hipFree(ws->wamb);
    if (ws->copy_in) hipStreamDestroy(ws->copy_in);
    if (ws->copy_out) hipStreamDestroy(ws->copy_out);
    for (int i = 0; i < 64; ++i) {
        if (ws->ev_in[i]) hipEventDestroy(ws->ev_in[i]);
        if (ws->ev_k[i]) hipEventDestroy(ws->ev_k[i]);
        if (ws->ev_out[i]) hipEventDestroy(ws->ev_out[i]);
    }
    if (ws->h_pipe) hipHostFree(ws->h_pipe);
    if (ws->d_pipe) hipFree(ws->d_pipe);
    if (ws->batch_seqs) hipFree(ws->batch_seqs);
    if (ws->batch_tiles) hipFree(ws->batch_tiles);
    if (ws->batch_offsets) hipFree(ws->batch_offsets);
    if (ws->h_batch) hipHostFree(ws->h_batch);
    if (ws->seg_table) hipFree(ws->seg_table);
    if (ws->seg_origin) hipFree(ws->seg_origin);
    if (ws->seg_first) hipFree(ws->seg_first);
    if (ws->seg_blk) hipFree(ws->seg_blk);
    if (ws->seg_starts) hipFree(ws->seg_starts);
    if (ws->seg_lens) hipFree(ws->seg_lens);
    if (ws->h_small) hipHostFree(ws->h_small);
    if (ws->d_amb) hipFree(ws->d_amb);
    if (ws->d_vals) hipFree(ws->d_vals);
    if (ws->d_one_min_keys) hipFree(ws->d_one_min_keys);
    if (ws->d_text_tables) hipFree(ws->d_text_tables);
    if (ws->d_text_tiles) hipFree(ws->d_text_tiles);
    if (ws->h_text_tables) hipHostFree(ws->h_text_tables);
    for (int i = 0; i < mm_workspace::kTextTableSlots; ++i)
        if (ws->ev_text_tables[i]) hipEventDestroy(ws->ev_text_tables[i]);
    if (ws->d_vbatch) hipFree(ws->d_vbatch);
    for (int i = 0; i < mm_workspace::kValuesBatchSlots; ++i) {
        if (ws->h_vbatch[i]) hipHostFree(ws->h_vbatch[i]);
        if (ws->ev_vbatch[i]) hipEventDestroy(ws->ev_vbatch[i]);
    }
    if (ws->own_stream && ws->stream) hipStreamDestroy(ws->stream);
    delete ws;
}

int mm_workspace_sync(mm_workspace_t *ws) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!ws) return MM_ERR_NULL;
    MM_HIP(hipStreamSynchronize(ws->stream));
    return MM_OK;
}

int mm_workspace_check(mm_workspace_t *ws) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!ws) return MM_ERR_NULL;
    MM_HIP(set_device(ws->device));
    MM_HIP(hipMemcpyAsync(ws->h_total + 2, ws->total + 2, sizeof(unsigned long long), hipMemcpyDeviceToHost,
                          ws->stream));
    MM_HIP(hipStreamSynchronize(ws->stream));
    const uint32_t code = (uint32_t)ws->h_total[2];
    ws->async_unchecked = false;
    if (code == 0) return MM_OK;
    MM_HIP(hipMemsetAsync(ws->total + 2, 0, sizeof(unsigned long long), ws->stream));
    if (code == 1u) {
        // workgroups were not dispatched in index order: every later run on this workspace takes its
        // tile ids from an atomic ticket; the caller repeats the runs since the last check
        ws->force_ticket = true;
        ws->no_split = true;
        ws->fasta_three_pass = true;
        g_last_error = "a look-back scan timed out in an asynchronous run: its output is invalid";
        return MM_ERR_ORDER;
    }
    if (code == 3u) {
        // the one-pass FASTA packer met a text whose lines are too short for its tables: the three-pass kernels take
        // over on this workspace; the caller repeats the calls since the last check (as for a look-back time-out)
        ws->fasta_three_pass = true;
        g_last_error = "mm_fasta_pack_device_async: lines too short for the one-pass packer; its output is invalid, "
                       "repeat the call (three-pass kernels from now on)";
        return MM_ERR_ORDER;
    }
    if (code == 6u) {
        g_last_error = kTextCountsRefused;
        return MM_ERR_CAPACITY;
    }
    if (code == 7u) {
        g_last_error = kLaneCountsRefused;
        return MM_ERR_CAPACITY;
    }
    if (code == 8u) {
        g_last_error = kOneMinCountsRefused;
        return MM_ERR_CAPACITY;
    }
    // (kernel errors 9 and 10: mm_bgzf_inflate_device_async, mm_bgzf.h)
    if (code == mm::kErrBgzfBlock) {
        g_last_error = "mm_bgzf_inflate_device_async: a BGZF block did not inflate (not deflate, or not ISIZE bytes of it); its "
                       "output slot is unspecified, every other block of the launch is complete";
        return MM_ERR_FORMAT;
    }
    if (code == mm::kErrBgzfTable) {
        g_last_error = "mm_bgzf_inflate_device_async: a BGZF block table entry lies beyond comp_bytes or out_capacity (or has "
                       "isize above 65536); nothing of that block was read or written";
        return MM_ERR_CAPACITY;
    }
    // (kernel error 11: mm_bgzf_crc32_device_async; the largest of the three, so it is what a queue with several reports)
    if (code == mm::kErrBgzfCrc) {
        g_last_error = "mm_bgzf_crc32_device_async: CRC32 mismatch: a BGZF block's text does not have the CRC32 of its gzip "
                       "trailer (d_status 15 names the block); the file is corrupt";
        return MM_ERR_FORMAT;
    }
    char buf[128];
    snprintf(buf, sizeof(buf), code == 2u   ? "kernel error 2: dynamic LDS does not lie behind the static LDS"
                               : code == 4u ? "kernel error 4: a skip-ambiguous launch without its LDS landing area"
                               : code == 5u ? "kernel error 5: the reads need more lanes than total_bases allows for"
                                            : "kernel error 0x%x (bad batch table)", code);
    g_last_error = buf;
    return MM_ERR_HIP;
}

int mm_workspace_force_generic(mm_workspace_t *ws, int on) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!ws) return MM_ERR_NULL;
    ws->force_generic = on != 0;
    return MM_OK;
}

int mm_workspace_set_blocks_per_lane(mm_workspace_t *ws, uint32_t nblk) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!ws) return MM_ERR_NULL;
    ws->nblk = nblk;
    return MM_OK;
}

int mm_workspace_enable_timing(mm_workspace_t *ws, int on) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!ws) return MM_ERR_NULL;
    ws->timing = on != 0;
    return MM_OK;
}

int mm_workspace_kernel_time(mm_workspace_t *ws, double *total_ms, uint64_t *launches, int reset) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!ws) return MM_ERR_NULL;
    MM_HIP(set_device(ws->device));
    int r = collect_timing(ws);
    if (r) return r;
    if (total_ms) *total_ms = ws->total_ms;
    if (launches) *launches = ws->launches;
    if (reset) {
        ws->total_ms = 0.0;
        ws->launches = 0;
    }
    return MM_OK;
}

int mm_workspace_last_path(const mm_workspace_t *ws) { return ws ? ws->last_path : 0; }
int mm_workspace_ticket_mode(const mm_workspace_t *ws) { return ws && ws->force_ticket ? 1 : 0; }
int mm_workspace_last_lane_table(const mm_workspace_t *ws) { return ws && ws->last_lane_table ? 1 : 0; }

// Diagnostics (no device needed when MM_TAPER_SLOTS names the workgroup slots): the launch plan of a run over
// n_windows windows - single sequence: out7 = {blocks per lane, tiles, taper_first, taper_per_level, taper_min_nblk,
// taper_start, windows per block of a tile}; batch (n_seqs > 0): the tile table itself, tile t = {seq, first window,
// blocks per lane}.  The CPU test-suite checks that the tiles tile every sequence exactly.
// the planner's view of a run: everything but the sizes is a placeholder (no device is touched)
static mm::RunArgs debug_plan_args(uint32_t w, int canonical_windows, int mode, uint64_t n_seqs, uint64_t n_windows0) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    const mm_plan_t plan = debug_plan(21, w, canonical_windows, mode);
    mm::RunArgs a{};
    set_packed_plan(a, &plan);
    a.ht.canonical = canonical_windows ? 1u : 0u;
    a.win_end = n_windows0;
    static uint32_t sk_marker, amb_marker;
    if (mode == 3) a.out.sk = &sk_marker;  // (only its being non-null matters to the planner)
    if (mode == 4) a.wamb = &amb_marker;
    a.batch_n = (uint32_t)n_seqs;
    a.work_windows = n_windows0;
    return a;
}

int mm_debug_launch_lds(uint32_t w, int canonical_windows, int mode, uint64_t n_windows, uint64_t *out2) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!out2 || w == 0) return MM_ERR_NULL;
    const mm::RunArgs a = debug_plan_args(w, canonical_windows, mode, 0, n_windows);
    unsigned long long o[2];
    mm::fused_debug_lds(a, o);
    out2[0] = o[0];
    out2[1] = o[1];
    return MM_OK;
}

int mm_debug_fixed_k_kernel(uint32_t k, uint32_t w, int canonical_windows) {
    return mm::fused_fixed_k(k, w, canonical_windows, canonical_windows) ? 1 : 0;
}

int mm_debug_kc_count(uint32_t w, uint32_t k, uint32_t kn, uint32_t jj, uint32_t group, const uint8_t *bytes, uint64_t n_bytes,
                      int64_t lane_base, uint32_t *count) {
    return mm::fused_kc_count(w, k, kn, jj, group, bytes, n_bytes, lane_base, count);
}

int mm_debug_pair_table(const mm_hasher_t *h, uint32_t out[1024]) {
    if (!h || !out) return MM_ERR_NULL;
    mm::fused_pair_table(make_tables(*h, 21), out);  // (k = 21: the k of the instance that walks with the table)
    return MM_OK;
}

static_assert(MM_WALK_TRAITS == mm::kWalkTraits, "the header's trait indices and fused_walk_traits list the same fields");
int mm_debug_walk_traits(uint32_t w, int canonical_windows, int mode, int super_kmers, int reads, int ambiguous, uint32_t *out,
                         int capacity) {
    if (w == 0 || mode < 0 || mode > 2) return 0;
    return mm::fused_walk_traits(w, canonical_windows != 0, (uint32_t)mode, super_kmers != 0, reads != 0, ambiguous != 0, out,
                                 capacity < 0 ? 0 : capacity);
}

int mm_debug_launch_plan(uint32_t w, int canonical_windows, int mode, uint64_t n_seqs, const uint64_t *n_windows,
                         uint64_t *out7, uint32_t *tile_seq, uint32_t *tile_win0, uint32_t *tile_nblk, uint64_t tile_capacity,
                         uint64_t *n_tiles) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!n_windows || w == 0) return MM_ERR_NULL;
    mm::RunArgs a = debug_plan_args(w, canonical_windows, mode, n_seqs, n_windows[0]);
    if (n_seqs == 0) {
        if (!out7) return MM_ERR_NULL;
        unsigned long long o[7];
        mm::fused_debug_plan(a, o);
        for (int i = 0; i < 7; ++i) out7[i] = o[i];
        return MM_OK;
    }
    a.work_windows = 0;
    for (uint64_t s = 0; s < n_seqs; ++s) a.work_windows += n_windows[s];
    std::vector<mm::BatchTile> tiles;
    uint32_t nb = 0;
    if (!mm::fused_batch_tiles(a, n_windows, n_seqs, tiles, &nb)) return MM_ERR_LEN_TOO_LARGE;
    if (n_tiles) *n_tiles = tiles.size();
    if (out7) out7[0] = nb;
    for (uint64_t t = 0; t < tiles.size() && t < tile_capacity; ++t) {
        if (tile_seq) tile_seq[t] = tiles[t].seq;
        if (tile_win0) tile_win0[t] = tiles[t].win0;
        if (tile_nblk) tile_nblk[t] = tiles[t].nblk;
    }
    return tiles.size() > tile_capacity ? MM_ERR_CAPACITY : MM_OK;
}

int mm_debug_lane_plan(uint32_t k, uint32_t w, int canonical_windows, int mode, uint64_t n_reads, uint64_t total_bases,
                       uint32_t blocks_per_lane, uint64_t *out6) {
    if (!out6 || w == 0 || k == 0) return MM_ERR_NULL;
    const mm_plan_t stand_in = debug_plan(k, w, canonical_windows, mode);
    mm::ReadsArgs a{};
    set_packed_plan(a, &stand_in);
    a.n_reads = n_reads;
    static uint32_t sk_marker, amb_marker;  // (only their being non-null matters to the planner)
    if (mode == 3) a.out.sk = &sk_marker;
    if (mode == 4) a.wamb = &amb_marker;
    mm::SegPlan plan;
    const int r = mm::fused_segments_plan(a, total_bases, blocks_per_lane, &plan);
    if (r) return MM_ERR_LEN_TOO_LARGE;
    out6[0] = plan.nblk;
    out6[1] = plan.S;
    out6[2] = plan.list_cap;
    out6[3] = plan.lds_bytes;
    out6[4] = plan.lanes_cap;
    out6[5] = plan.tiles;
    return MM_OK;
}

int mm_debug_last_lane_table(mm_workspace_t *ws, uint32_t *out4, uint64_t capacity, uint64_t *n_lanes) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!ws || !n_lanes) return MM_ERR_NULL;
    *n_lanes = ws->last_lane_table ? ws->last_lanes : 0;
    if (!ws->last_lane_table || !out4 || capacity == 0) return MM_OK;
    MM_HIP(set_device(ws->device));
    const uint64_t m = capacity < ws->last_lanes ? capacity : ws->last_lanes;
    MM_HIP(hipMemcpyAsync(out4, ws->seg_table, m * sizeof(mm::LaneSeg), hipMemcpyDeviceToHost, ws->stream));
    MM_HIP(hipStreamSynchronize(ws->stream));
    return MM_OK;
}

uint64_t mm_fused_overread_bytes(void) { return mm::fused_overread_bytes(); }

int mm_text_prebuilt_window_sizes(int canonical_windows, uint32_t *out, int capacity) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    (void)canonical_windows;  // (the same sizes for both strands)
    return mm::text_prebuilt_windows(out, capacity < 0 ? 0 : capacity);
}

int mm_prebuilt_window_sizes(int canonical_windows, int reads_mode, uint32_t *out, int capacity) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    return mm::fused_prebuilt_windows(canonical_windows != 0, reads_mode != 0, out, capacity < 0 ? 0 : capacity);
}

int mm_prebuilt_flavour_window_sizes(int canonical_windows, int reads_mode, mm_mode_t mode, int super_kmers, uint32_t *out,
                                     int capacity) {
    if ((int)mode < 0 || (int)mode > 2) return 0;
    return mm::fused_prebuilt_flavour_windows(canonical_windows != 0, reads_mode != 0, (uint32_t)mode, super_kmers != 0, out,
                                              capacity < 0 ? 0 : capacity);
}

int mm_jit_stats(uint64_t out[4]) {
    if (!out) return MM_ERR_NULL;
    mm::jit_stats(out);
    return MM_OK;
}

// Builder::run (src/lib.rs:378) is compiled code whose first call costs what every call costs; here a plan's first run
// loads its kernels' code objects and may compile one.  mm_plan_prepare does exactly that part of a first run - through
// the launcher's own choice of kernel, so the two cannot disagree - and launches nothing.
int mm_plan_prepare(const mm_plan_t *plan, mm_workspace_t *ws, uint32_t what, mm_prepare_report_t *report) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (report) *report = mm_prepare_report_t{0, 0, 0, 0};
    if (!plan || !ws) return MM_ERR_NULL;
    if (what & ~(uint32_t)(MM_PREPARE_SEQUENCE | MM_PREPARE_READS | MM_PREPARE_SUPERKMERS)) return MM_ERR_BAD_MODE;
    if ((what & MM_PREPARE_SUPERKMERS) && plan->mode != MM_MINIMIZERS) return MM_ERR_BAD_MODE;  // src/lib.rs:339
    const bool sequence = (what & MM_PREPARE_SEQUENCE) != 0, reads = (what & MM_PREPARE_READS) != 0;
    if (!sequence && !reads) return MM_OK;
    MM_HIP(set_device(ws->device));
    mm::PrepareCounts c;
    if (plan->text) {
        // byte text: every kernel is prebuilt - the fused text kernel with its batch twin, or the generic family's
        if (!ws->force_generic && mm::text_walk_supported(plan->k, plan->w))
            MM_HIP(mm::text_walk_prepare(plan->w, plan->canonical_windows != 0, plan->tt.canonical != 0, plan->mode, &c.kernels));
        else
            MM_HIP(mm::generic_prepare(true, &c.kernels));
    } else if (ws->force_generic || plan->w > mm::kJitMaxW) {
        // (w > kJitMaxW: no fused kernel exists for any plan, the prebuilt generic family is the only path - nothing is missing)
        MM_HIP(mm::generic_prepare(false, &c.kernels));
    } else {
        MM_HIP(mm::fused_prepare(plan->k, plan->w, plan->canonical_windows, (int)plan->ht.canonical, plan->mode, sequence, reads,
                                 (what & MM_PREPARE_SUPERKMERS) != 0, &c));
        if (c.unavailable) {
            // such runs take the generic family (reads one launch per read): have it loaded, and say why
            MM_HIP(mm::generic_prepare(false, &c.kernels));
            g_last_error = std::string("fused kernel unavailable, generic family used: ") + mm::fused_unavailable_reason();
        }
    }
    if (report) *report = mm_prepare_report_t{c.kernels, c.compiled, c.from_disk, c.unavailable};
    return MM_OK;
}

// Ambiguity bits of a PackedNSeq as they cross the ABI (null d_amb = plain PackedSeq).
struct AmbArgs {
    const void *d_amb;
    uint64_t bytes;
    uint64_t bit_offset;
};

// ---- What the caller of a run passed: one plain struct per family.  The exported wrappers fill one by field name, the
// checks, *_async_impl and *_sync functions take (plan, ws, call).  Fields that a wrapper does not name are null / 0.
struct SeqCall {  // one sequence: mm_run_device*, mm_run_skip_ambiguous_device*, and every loop over reads or sequences
    const void *d_packed;
    uint64_t packed_bytes, base_offset, n_bases, win_begin, win_end;
    uint32_t *d_out_pos, *d_out_sk;
    uint64_t capacity;
    uint64_t *d_count;
    // keep the running total of the previous launch, so that consecutive runs write their outputs back to back (the
    // kernels take the total as the carry-in of their first tile)
    bool append;
    const AmbArgs *amb;  // null: a plain PackedSeq
    // synchronous callers: *host_total_written is set when the kernel stores the total into a page-locked host word
    // itself - ws->h_total[0], or host_word_dev (as the device addresses it: the pipelined host path gives every chunk
    // its own)
    bool *host_total_written;
    unsigned long long *host_word_dev;
};
struct ReadsCall {  // reads of one packed buffer at a fixed stride, or (d_read_starts) back to back
    const void *d_packed;
    uint64_t packed_bytes, base_offset, n_reads;
    uint32_t read_stride, read_len;  // (back to back: read_len is the longest read to expect, read_stride is not used)
    const uint32_t *d_read_lens;
    // reads packed back to back (round 4): read r = bases [starts[r], starts[r + 1]) of the buffer, n_reads + 1 device
    // entries; total_bases = starts[n_reads], which the caller knows from the packer's counts
    const uint64_t *d_read_starts;
    uint64_t total_bases;
    uint32_t *d_out_pos, *d_out_sk;
    uint64_t capacity;
    uint64_t *d_out_offsets, *d_count;
    const AmbArgs *amb;
};
struct ReadsCountsCall {  // reads back to back with {bases, records} in device memory (d_counts)
    const void *d_packed;
    uint64_t packed_bytes, base_offset, max_bases, max_records;
    const uint64_t *d_read_starts, *d_counts;
    uint32_t *d_out_pos, *d_out_sk;
    uint64_t capacity;
    uint64_t *d_out_offsets, *d_count;
    const AmbArgs *amb;
};
struct BatchCall {  // separately allocated sequences (host arrays of n_seqs entries; base_offsets may be null)
    uint64_t n_seqs;
    const void *const *d_packed;
    const uint64_t *packed_bytes, *base_offsets, *n_bases;
    uint32_t *d_out_pos, *d_out_sk;
    uint64_t capacity;
};
struct TextCall {  // one byte text
    const void *d_text;
    uint64_t text_bytes, n, win_begin, win_end;
    uint32_t *d_out_pos, *d_out_sk;
    uint64_t capacity;
    uint64_t *d_count;
};
struct TextBatchCall {  // records of one byte text
    const void *d_text;
    uint64_t text_bytes, n_records;
    const uint64_t *d_starts;
    uint64_t n_chars;
    uint32_t *d_out_pos, *d_out_sk;
    uint64_t capacity;
    uint64_t *d_out_offsets, *d_count;
};
struct TextBatchCountsCall {  // the same with {characters, records} in device memory (d_counts)
    const void *d_text;
    uint64_t text_bytes, max_chars, max_records;
    const uint64_t *d_starts, *d_counts;
    uint32_t *d_out_pos, *d_out_sk;
    uint64_t capacity;
    uint64_t *d_out_offsets, *d_count;
};

// Fills ws->wamb with the window ambiguity bits of windows [win_begin - 1, win_end) of a
// sequence / buffer span of `span_bases` bases whose windows are l bases long.
static int prepare_window_ambiguity(mm_workspace_t *ws, const AmbArgs &amb, uint64_t span_bases,
                                    uint32_t l, uint64_t win_begin, uint64_t win_end,
                                    uint32_t *out_dwords) {
    if (!amb.d_amb) return MM_ERR_NULL;
    const uintptr_t a = reinterpret_cast<uintptr_t>(amb.d_amb);
    const uint64_t byte_shift = a & 3u;
    const uint64_t bit0 = amb.bit_offset + 8 * byte_shift;
    const uint64_t n_dwords = (byte_shift + amb.bytes + 3) / 4;
    if (n_dwords == 0 || n_dwords >= (1ull << 32)) return MM_ERR_LEN_TOO_LARGE;
    if ((bit0 + span_bases + 31) / 32 > n_dwords) return MM_ERR_CAPACITY;
    // (pad dwords: read by the one-block-ahead prefetch of the last lanes - two for the 8-byte views, four for the
    // 16-byte loads of the large windows' walk, which must lie INSIDE the buffer descriptor's range as a whole)
    const uint64_t kPad = 8;
    const uint64_t need = (win_end + 31) / 32 + kPad;
    int r = grow(ws->wamb, ws->wamb_dwords, need, sizeof(uint32_t));
    if (r) return r;
    MM_HIP(hipMemsetAsync(ws->wamb + (need - kPad), 0, kPad * sizeof(uint32_t), ws->stream));
    if (mm::launch_window_ambiguity(reinterpret_cast<const uint32_t *>(a - byte_shift), (uint32_t)n_dwords,
                                    bit0, l, win_begin, win_end, ws->wamb, ws->stream))
        return hip_fail(hipGetLastError(), "window_ambiguity");
    *out_dwords = (uint32_t)need;
    return MM_OK;
}

static int run_device_async_impl(const mm_plan_t *plan, mm_workspace_t *ws, const SeqCall &c) {
    uint64_t win_end = c.win_end, capacity = c.capacity;
    // Stream operations of one run (round 4): the fused kernel alone.  Its look-back words are epoch-tagged (no
    // clear), a run that does not append ignores the old total (no clear), and its last tile stores the total to
    // d_count and - for the synchronous entry points, host_total_written != null - to the page-locked host word
    // ws->h_total[0] as well (no copies).  The split path, the generic family and empty runs keep the cleared
    // total + copy protocol of rounds 1-3.  The per-run error word total[1] is NOT cleared here any more: the entry
    // points that read it clear it themselves.
    if (c.host_total_written) *c.host_total_written = false;
    if (!plan || !ws) return MM_ERR_NULL;
    if (c.n_bases >= (1ull << 32)) return MM_ERR_LEN_TOO_LARGE;
    if (c.d_out_sk && plan->mode != MM_MINIMIZERS) return MM_ERR_BAD_MODE;  // src/lib.rs:339
    if (c.amb) {
        // run_skip_ambiguous_windows exists on canonical builders only and has no super-k-mer
        // flavour (src/lib.rs:451-496; assert src/minimizers.rs:176)
        if (!plan->canonical_windows) return MM_ERR_HASHER_NOT_CANONICAL;
        if (c.d_out_sk) return MM_ERR_BAD_MODE;
    }
    if (!c.d_out_pos) capacity = 0;
    MM_HIP(set_device(ws->device));
    const uint64_t l = (uint64_t)plan->k + plan->w - 1;
    const uint64_t n_w = c.n_bases >= l ? c.n_bases - l + 1 : 0;
    if (win_end > n_w) win_end = n_w;
    bool total_cleared = false, count_stored = false;
    auto clear_total = [&]() -> int {  // (families that take *total as their carry-in; with it the per-run error word)
        if (!c.append && !total_cleared) MM_HIP(hipMemsetAsync(ws->total, 0, 2 * sizeof(unsigned long long), ws->stream));
        total_cleared = true;
        return MM_OK;
    };
    if (c.win_begin < win_end) {
        if (!c.d_packed) return MM_ERR_NULL;
        mm::RunArgs a{};
        int r = make_view(c.d_packed, c.packed_bytes, c.base_offset, c.n_bases, &a.seq);
        if (r) return r;
        set_packed_plan(a, plan);
        a.win_begin = c.win_begin;
        a.win_end = win_end;
        a.out = out_params(ws, c.d_out_pos, c.d_out_sk, capacity);
        a.nblk = ws->nblk;
        a.use_ticket = use_ticket(ws);
        a.work_windows = win_end - c.win_begin;
        a.append = c.append;
        if (c.amb) {
            r = prepare_window_ambiguity(ws, *c.amb, c.n_bases, (uint32_t)l, c.win_begin, win_end, &a.wamb_dwords);
            if (r) return r;
            a.wamb = ws->wamb;
        }
        bool fused = !ws->force_generic &&
                     mm::fused_supported(plan->k, plan->w, plan->canonical_windows,
                                         (int)plan->ht.canonical);
        TimedLaunch timed(ws);  // (one pair for whichever launch finally runs: split, fused, or generic after lr == -2)
        r = timed.arm(a);
        if (r) return r;
        int lr = 0;
        bool split = false;
#ifdef MM_EXPERIMENTS
        if (fused && !ws->no_split && mm::split_wanted(a)) {
            // split path: the walk dumps its lists, expander workgroups on a second stream write the positions
            uint64_t tiles = 0, dump_bytes = 0;
            mm::split_requirements(a, &tiles, &dump_bytes);
            if (tiles) {
                r = prepare_split(ws, tiles, dump_bytes);
                if (r) return r;
                r = clear_total();
                if (r) return r;
                a.out.status = nullptr;
                lr = mm::launch_split(a, ws->split, ws->stream);
                split = lr == 0;
                if (lr == -2) lr = 0;  // no walk kernel for this plan: the fused kernel below
            }
        }
#endif
        if (fused && !split && lr == 0) {
            r = grow_status(ws, mm::fused_status_words(a));
            if (r) return r;
            a.out.status = ws->status;
            a.status_avail = ws->status_words;
            r = next_status_epoch(ws, &a.status_epoch);
            if (r) return r;
            a.out.count_out = reinterpret_cast<unsigned long long *>(c.d_count);
            a.out.total_host = c.host_total_written ? (c.host_word_dev ? c.host_word_dev : ws->h_total_dev) : nullptr;
            lr = mm::launch_fused(a, ws->stream);
            if (lr == 0) {
                count_stored = c.d_count != nullptr;
                if (c.host_total_written && a.out.total_host) *c.host_total_written = true;
            }
            a.out.count_out = a.out.total_host = nullptr;
            if (lr == -2) {
                // no prebuilt instance and the run-time specialisation is unavailable: generic family
                g_last_error = std::string("fused kernel unavailable, generic family used: ") +
                               mm::fused_unavailable_reason();
                fused = false;
            }
        }
        if (!fused) {
            const uint64_t nwin = win_end - c.win_begin;
            a.generic_round_windows = nwin < (1ull << 24) ? nwin : (1ull << 24);
            r = grow_bytes(ws->scratch, ws->scratch_bytes, mm::generic_scratch_bytes(a.generic_round_windows, plan->w));
            if (r) return r;
            a.scratch = ws->scratch;
            r = grow_status(ws, mm::generic_status_words(a.generic_round_windows));
            if (r) return r;
            r = clear_total();
            if (r) return r;
            a.out.status = ws->status;
            ws->status_dirty = true;  // (the generic family clears and writes untagged words)
            lr = mm::launch_generic(a, ws->stream);
        }
        if (lr != 0) return launch_failed();
        timed.done(fused ? (split ? MM_PATH_SPLIT : MM_PATH_FUSED) : MM_PATH_GENERIC);
    } else {
        const int r = clear_total();  // an empty run: the total is what it was (append) or 0
        if (r) return r;
    }
    if (c.d_count && !count_stored)
        MM_HIP(hipMemcpyAsync(c.d_count, ws->total, sizeof(unsigned long long), hipMemcpyDeviceToDevice,
                              ws->stream));
    return MM_OK;
}

int mm_run_device_async(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed,
                        uint64_t packed_bytes, uint64_t base_offset, uint64_t n_bases,
                        uint64_t win_begin, uint64_t win_end, uint32_t *d_out_pos,
                        uint32_t *d_out_sk, uint64_t capacity, uint64_t *d_count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (const int bad = dna_plan_only(plan)) return bad;
    if (ws) ws->async_unchecked = true;
    return run_device_async_impl(plan, ws, {.d_packed = d_packed, .packed_bytes = packed_bytes, .base_offset = base_offset,
                                            .n_bases = n_bases, .win_begin = win_begin, .win_end = win_end,
                                            .d_out_pos = d_out_pos, .d_out_sk = d_out_sk, .capacity = capacity,
                                            .d_count = d_count});
}

// Lane-table launch (round 6; mm_lanes.hip): reads / sequences of ANY lengths in ONE launch of the reads-mode kernel at
// full lane occupancy.  `a` is the filled ReadsArgs of the run (status words and epoch are set here), `total_bases` the
// bases of all reads together.  Returns 0, a negative MM_ERR_* code, or 1 when no lane-table launch can be had
// (no kernel, no lane length that fits): the caller keeps its other paths.
// MM_LANE_TABLE=0 switches the launches off (A/B: the per-read lanes / per-sequence tiles of rounds 2-5), =1 takes them
// for every reads / batch run; results are identical either way.
static int lane_table_policy() {
    const char *e = mm::mm_env("MM_LANE_TABLE");
    return e ? (e[0] == '0' ? 0 : 1) : -1;
}
static int run_lane_table(mm_workspace_t *ws, mm::ReadsArgs &a, const mm::SegSource &src, uint64_t total_bases) {
    mm::SegPlan plan;
    const int pr = mm::fused_segments_plan(a, total_bases, ws->nblk, &plan);
    if (pr) return 1;
    int r = grow(ws->seg_table, ws->seg_table_n, plan.lanes_cap, sizeof(mm::LaneSeg));
    if (r) return r;
    r = grow(ws->seg_origin, ws->seg_origin_n, plan.tiles, sizeof(uint32_t));
    if (r) return r;
    r = grow(ws->seg_first, ws->seg_first_n, a.n_reads + 1, sizeof(uint32_t));
    if (r) return r;
    r = grow(ws->seg_blk, ws->seg_blk_n, mm::lane_table_blocks(a.n_reads) + 1, sizeof(uint32_t));
    if (r) return r;
    r = grow_status(ws, (plan.tiles + 8) * mm::fused_status_stride());
    if (r) return r;
    a.out.status = ws->status;
    r = next_status_epoch(ws, &a.status_epoch);
    if (r) return r;
    mm::SegBuffers b{ws->seg_table, ws->seg_origin, ws->seg_first, ws->seg_blk};
    TimedLaunch timed(ws);
    r = timed.arm(a);
    if (r) return r;
    const int lr = mm::launch_fused_segments(a, src, plan, b, ws->stream);
    if (lr == -1) return launch_failed();
    if (lr != 0) return 1;
    timed.done(MM_PATH_FUSED);
    ws->last_lane_table = true;
    ws->last_lanes = plan.lanes_cap;
    return MM_OK;
}

// Batch mode of the fused kernel: every sequence is cut into tiles, one launch covers all tiles of
// all sequences (a tile reads its sequence from a device table), so a batch of thousands of contigs
// costs one launch instead of one per sequence.  Returns MM_BATCH_FALLBACK when the plan has no
// fused kernel (then the caller loops over the sequences).
static const int MM_BATCH_FALLBACK = 1;
static const int MM_BATCH_REDO = 2;

// Round 5: the launch is split into an ISSUE half (tables, uploads, the launch, the copies of the offsets and the result
// words into page-locked memory: nothing waits) and a FINISH half (wait, judge, patch the offsets of empty sequences), so
// that a device group issues one batch launch per entry from the calling thread and then waits for them in turn - the
// model of mm_run_sharded_device - instead of a host thread per entry.
struct BatchIssue {
    std::vector<mm::BatchSeq> seqs;        // (host copies of the tables: alive until the uploads have been waited for)
    std::vector<mm::BatchTile> tile_seq;
    std::vector<unsigned long long> starts;  // lane-table launches: where every sequence starts in the common span, its length
    std::vector<uint32_t> lens;
    uint64_t n_seqs = 0;
    bool launched = false;                 // false: nothing was queued (no tile at all): every offset is 0
};

static int batch_issue(const mm_plan_t *plan, mm_workspace_t *ws, const BatchCall &c, BatchIssue *bi) {
    uint64_t capacity = c.capacity;
    bi->n_seqs = c.n_seqs;
    bi->launched = false;
    ws->last_lane_table = false;  // (also when the batch falls back to one launch per sequence)
    if (ws->force_generic || c.n_seqs == 0 || c.n_seqs >= (1ull << 32) ||
        !mm::fused_supported(plan->k, plan->w, plan->canonical_windows, (int)plan->ht.canonical))
        return MM_BATCH_FALLBACK;
    if (c.d_out_sk && plan->mode != MM_MINIMIZERS) return MM_ERR_BAD_MODE;
    if (!c.d_out_pos) capacity = 0;
    mm::RunArgs a{};
    set_packed_plan(a, plan);
    a.out = out_params(ws, c.d_out_pos, c.d_out_sk, capacity);
    a.nblk = ws->nblk;
    a.batch_n = (uint32_t)c.n_seqs;
    const uint64_t l = (uint64_t)plan->k + plan->w - 1;
    // lane length: a tile should not be much larger than a typical sequence of the batch (every
    // sequence starts a tile of its own), nor the batch too short to fill the chip
    uint64_t nonempty = 0;
    for (uint64_t s = 0; s < c.n_seqs; ++s) {
        a.work_windows += c.n_bases[s] >= l ? c.n_bases[s] - l + 1 : 0;
        nonempty += c.n_bases[s] >= l ? 1 : 0;
    }
    if (nonempty) {
        const uint64_t per_seq = a.work_windows / nonempty * 1024ull;
        if (per_seq < a.work_windows) a.work_windows = per_seq ? per_seq : 1;
    }
    std::vector<mm::BatchSeq> &seqs = bi->seqs;
    std::vector<mm::BatchTile> &tile_seq = bi->tile_seq;
    seqs.assign(c.n_seqs, mm::BatchSeq{nullptr, 0, 0, 0, 0, {0, 0}});
    tile_seq.clear();
    std::vector<uint64_t> nws(c.n_seqs);
    for (uint64_t s = 0; s < c.n_seqs; ++s) {
        if (c.n_bases[s] >= (1ull << 32)) return MM_ERR_LEN_TOO_LARGE;
        nws[s] = c.n_bases[s] >= l ? c.n_bases[s] - l + 1 : 0;
    }
    // Round 6: batches of SHORT sequences take a lane-table launch of the reads-mode kernel (mm_lanes.hip) - a tile's 256
    // lanes are any 256 consecutive segments of the batch, where the tile table below gives every sequence tiles of its
    // own (a 10 kbp contig fills 33 of 256 lanes).  Needs all sequences inside ONE ALLOCATION and one span of < 2^32 bases from the lowest
    // pointer (one allocation, the FASTA packer's buffer); long contigs keep their tiles (tapered tail, sequence kernel).
    if (nonempty && lane_table_policy() != 0) {
        mm::RunArgs probe = a;
        probe.work_windows = 0;
        const uint64_t tile_w = mm::fused_tile_windows(probe);  // windows of a default tile
        uint64_t total_w = 0;
        for (uint64_t s = 0; s < c.n_seqs; ++s) total_w += nws[s];
        // (the crossover, measured on 1 Gbp of equal contigs - tools/gpu_batch_crossover.py, profiles/r06_batch_crossover.txt: the
        // lane table wins up to 500 kbp per contig and the per-sequence tiles from 1 Mbp on, at w = 11 - 6 and 13 tiles per
        // contig - as at w = 51 - 1.4 and 2.8: eight tiles or 750 k windows, whichever is less)
        const uint64_t per_seq_limit = 8 * tile_w < 750000ull ? 8 * tile_w : 750000ull;
        const bool short_seqs = total_w / nonempty < per_seq_limit;
        if ((short_seqs || lane_table_policy() == 1) &&
            mm::fused_reads_supported(plan->w, plan->canonical_windows, (int)plan->ht.canonical, plan->mode, c.d_out_sk != nullptr)) {
            uintptr_t lo = ~(uintptr_t)0, hi = 0;
            uint32_t max_len = 0;
            for (uint64_t s = 0; s < c.n_seqs; ++s) {
                if (nws[s] == 0) continue;
                if (!c.d_packed[s]) return MM_ERR_NULL;
                const uintptr_t p0 = reinterpret_cast<uintptr_t>(c.d_packed[s]);
                if ((((c.base_offsets ? c.base_offsets[s] : 0) + c.n_bases[s] + 3) / 4) > c.packed_bytes[s]) return MM_ERR_CAPACITY;
                lo = p0 < lo ? p0 : lo;
                hi = p0 + c.packed_bytes[s] > hi ? p0 + c.packed_bytes[s] : hi;
                if (c.n_bases[s] > max_len) max_len = (uint32_t)c.n_bases[s];
            }
            const uint64_t span_bytes = hi - lo;
            // ONE descriptor covers the span from the lowest sequence to the end of the highest, and a lane's loads run a few
            // KB past its sequence's end (fused_overread_bytes): everything between the sequences has to be mapped memory - true
            // inside one allocation (the FASTA / FASTQ packer's buffer, slices of one tensor), not between allocations.  The
            // per-sequence tiles below clamp every load to its own sequence's bytes and need no such thing.
            bool one_allocation = false;
            {
                hipDeviceptr_t abase = nullptr;
                size_t asize = 0;
                if (hipMemGetAddressRange(&abase, &asize, reinterpret_cast<hipDeviceptr_t>(lo)) == hipSuccess) {
                    const uintptr_t a0 = reinterpret_cast<uintptr_t>(abase);
                    one_allocation = lo >= a0 && hi <= a0 + asize;
                } else {
                    (void)hipGetLastError();
                }
            }
            if (one_allocation && span_bytes < (1ull << 30) - 64) {
                bi->starts.assign(c.n_seqs + 1, 0);
                bi->lens.assign(c.n_seqs, 0);
                uint64_t total_bases = 0;
                for (uint64_t s = 0; s < c.n_seqs; ++s) {
                    if (nws[s] == 0) continue;  // (no window: an empty lane; its start is never read from)
                    bi->starts[s] = (reinterpret_cast<uintptr_t>(c.d_packed[s]) - lo) * 4ull + (c.base_offsets ? c.base_offsets[s] : 0);
                    bi->lens[s] = (uint32_t)c.n_bases[s];
                    total_bases += c.n_bases[s];
                }
                mm::ReadsArgs ra{};
                int r = make_view(reinterpret_cast<const void *>(lo), span_bytes, 0, span_bytes * 4ull, &ra.seq);
                if (r == MM_OK) {
                    r = grow(ws->seg_starts, ws->seg_starts_n, c.n_seqs + 1, sizeof(unsigned long long));
                    if (r) return r;
                    r = grow(ws->seg_lens, ws->seg_lens_n, c.n_seqs, sizeof(uint32_t));
                    if (r) return r;
                    r = grow(ws->batch_offsets, ws->batch_offsets_n, c.n_seqs + 1, sizeof(unsigned long long));
                    if (r) return r;
                    r = grow_h_batch(ws, c.n_seqs + 1);
                    if (r) return r;
                    MM_HIP(hipMemcpyAsync(ws->seg_starts, bi->starts.data(), (c.n_seqs + 1) * sizeof(unsigned long long),
                                          hipMemcpyHostToDevice, ws->stream));
                    MM_HIP(hipMemcpyAsync(ws->seg_lens, bi->lens.data(), c.n_seqs * sizeof(uint32_t), hipMemcpyHostToDevice, ws->stream));
                    set_packed_plan(ra, plan);
                    ra.n_reads = c.n_seqs;
                    ra.read_len = max_len;
                    ra.read_offsets = ws->batch_offsets;
                    ra.out = a.out;
                    ra.use_ticket = use_ticket(ws);
                    MM_HIP(hipMemsetAsync(ws->total, 0, 2 * sizeof(unsigned long long), ws->stream));
                    const mm::SegSource src{ws->seg_starts, ws->seg_lens, 0, max_len};
                    r = run_lane_table(ws, ra, src, total_bases);
                    if (r < 0) return r;
                    if (r == 0) {
                        MM_HIP(hipMemcpyAsync(ws->h_batch, ws->batch_offsets, (c.n_seqs + 1) * sizeof(unsigned long long),
                                              hipMemcpyDeviceToHost, ws->stream));
                        MM_HIP(hipMemcpyAsync(ws->h_total, ws->total, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ws->stream));
                        bi->launched = true;
                        return MM_OK;
                    }
                }
            }
        }
    }
    {
        // the tile table (mm_fused.hip): whole tiles per sequence, lanes sized for whole rounds of resident
        // workgroups or - long batches - default lanes and a tapered last round
        uint32_t nb = 0;
        if (!mm::fused_batch_tiles(a, nws.data(), c.n_seqs, tile_seq, &nb)) return MM_BATCH_FALLBACK;
        a.nblk = nb;
    }
    for (uint64_t s = 0; s < c.n_seqs; ++s) {
        const uint64_t nw = nws[s];
        mm::BatchSeq &b = seqs[s];
        if (nw == 0) continue;
        if (!c.d_packed[s]) return MM_ERR_NULL;
        mm::SeqView v;
        int r = make_view(c.d_packed[s], c.packed_bytes[s], c.base_offsets ? c.base_offsets[s] : 0, c.n_bases[s], &v);
        if (r) return r;
        b.d = v.d;
        b.n_dwords = v.n_dwords;
        b.base0 = v.base0;
        b.n_windows = (uint32_t)nw;
    }
    const uint64_t n_tiles = tile_seq.size();
    if (n_tiles == 0) return MM_OK;  // (launched stays false: every offset is 0)
    int r = grow(ws->batch_seqs, ws->batch_seqs_n, c.n_seqs, sizeof(mm::BatchSeq));
    if (r) return r;
    r = grow(ws->batch_tiles, ws->batch_tiles_n, n_tiles, sizeof(mm::BatchTile));
    if (r) return r;
    r = grow(ws->batch_offsets, ws->batch_offsets_n, c.n_seqs + 1, sizeof(unsigned long long));
    if (r) return r;
    r = grow_h_batch(ws, c.n_seqs + 1);
    if (r) return r;
    MM_HIP(hipMemcpyAsync(ws->batch_seqs, seqs.data(), c.n_seqs * sizeof(mm::BatchSeq), hipMemcpyHostToDevice,
                          ws->stream));
    MM_HIP(hipMemcpyAsync(ws->batch_tiles, tile_seq.data(), n_tiles * sizeof(mm::BatchTile), hipMemcpyHostToDevice,
                          ws->stream));
    a.batch_seqs = ws->batch_seqs;
    a.batch_tile_seq = ws->batch_tiles;
    a.batch_offsets = ws->batch_offsets;
    a.batch_tiles = n_tiles;
    r = grow_status(ws, (n_tiles + 8) * mm::fused_status_stride());
    if (r) return r;
    a.out.status = ws->status;
    a.status_avail = ws->status_words;
    a.use_ticket = use_ticket(ws);
    r = next_status_epoch(ws, &a.status_epoch);
    if (r) return r;
    MM_HIP(hipMemsetAsync(ws->total, 0, 2 * sizeof(unsigned long long), ws->stream));
    MM_HIP(hipMemsetAsync(ws->batch_offsets, 0xFF, (c.n_seqs + 1) * sizeof(unsigned long long), ws->stream));
    TimedLaunch timed(ws);
    r = timed.arm(a);
    if (r) return r;
    const int lr = mm::launch_fused(a, ws->stream);
    if (lr == -2) return MM_BATCH_FALLBACK;
    if (lr != 0) return launch_failed();
    timed.done(MM_PATH_FUSED);
    MM_HIP(hipMemcpyAsync(ws->h_batch, ws->batch_offsets, (c.n_seqs + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                          ws->stream));
    MM_HIP(hipMemcpyAsync(ws->h_total, ws->total, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ws->stream));
    bi->launched = true;
    return MM_OK;
}

// The other half: wait for an issued batch launch.  Returns MM_OK, MM_BATCH_REDO (a look-back spin ran out: the workspace
// is in ticket mode now, issue the batch again), MM_ERR_CAPACITY (the true total is in out_offsets[n_seqs]) or another error.
static int batch_finish(mm_workspace_t *ws, BatchIssue *bi, bool has_pos, uint64_t capacity, uint64_t *out_offsets) {
    const uint64_t n_seqs = bi->n_seqs;
    if (!bi->launched) {
        for (uint64_t s = 0; s <= n_seqs; ++s) out_offsets[s] = 0;
        return MM_OK;
    }
    MM_HIP(hipStreamSynchronize(ws->stream));
    bi->seqs.clear();
    bi->tile_seq.clear();
    bi->starts.clear();
    bi->lens.clear();
    const int je = judge_run_error(ws);
    if (je < 0) return je;
    if (je == 1) return MM_BATCH_REDO;  // (the workspace is in ticket mode now)
    // sequences without a window own no tile: their slice is empty and starts where the next one does
    unsigned long long *offs = ws->h_batch;
    offs[n_seqs] = ws->h_total[0];
    for (uint64_t s = n_seqs; s-- > 0;)
        if (offs[s] == ~0ull) offs[s] = offs[s + 1];
    for (uint64_t s = 0; s <= n_seqs; ++s) out_offsets[s] = offs[s];
    if (has_pos && out_offsets[n_seqs] > capacity) return MM_ERR_CAPACITY;
    return MM_OK;
}

static int run_batch_one_launch(const mm_plan_t *plan, mm_workspace_t *ws, const BatchCall &c, uint64_t *out_offsets) {
    BatchIssue bi;
    for (int attempt = 0; attempt < 2; ++attempt) {
        int r = batch_issue(plan, ws, c, &bi);
        if (r) return r;
        r = batch_finish(ws, &bi, c.d_out_pos != nullptr, c.capacity, out_offsets);
        if (r != MM_BATCH_REDO) return r;
    }
    g_last_error = "look-back scan timed out in ticket mode";
    return MM_ERR_HIP;
}

int mm_run_batch_device(const mm_plan_t *plan, mm_workspace_t *ws, uint64_t n_seqs,
                        const void *const *d_packed, const uint64_t *packed_bytes,
                        const uint64_t *base_offsets, const uint64_t *n_bases,
                        uint32_t *d_out_pos, uint32_t *d_out_sk, uint64_t capacity,
                        uint64_t *out_offsets) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (const int bad = dna_plan_only(plan)) return bad;
    if (!plan || !ws || !out_offsets) return MM_ERR_NULL;
    if (n_seqs && (!d_packed || !packed_bytes || !n_bases)) return MM_ERR_NULL;
    MM_HIP(set_device(ws->device));
    {
        int r = run_batch_one_launch(plan, ws, {.n_seqs = n_seqs, .d_packed = d_packed, .packed_bytes = packed_bytes,
                                                .base_offsets = base_offsets, .n_bases = n_bases, .d_out_pos = d_out_pos,
                                                .d_out_sk = d_out_sk, .capacity = capacity}, out_offsets);
        if (r != MM_BATCH_FALLBACK) return r;
    }
    for (int attempt = 0; attempt < 2; ++attempt) {
        // running totals after each sequence, read back once at the end
        unsigned long long *h = nullptr;
        MM_HIP(hipHostMalloc(reinterpret_cast<void **>(&h), (n_seqs + 1) * sizeof(unsigned long long),
                             hipHostMallocDefault));
        int r = MM_OK;
        // (the runs below do not clear the per-run error word themselves)
        if (hipMemsetAsync(ws->total, 0, 2 * sizeof(unsigned long long), ws->stream) != hipSuccess) r = MM_ERR_HIP;
        for (uint64_t s = 0; s < n_seqs && r == MM_OK; ++s) {
            r = run_device_async_impl(plan, ws, {.d_packed = d_packed[s], .packed_bytes = packed_bytes[s],
                                                 .base_offset = base_offsets ? base_offsets[s] : 0, .n_bases = n_bases[s],
                                                 .win_end = UINT64_MAX, .d_out_pos = d_out_pos, .d_out_sk = d_out_sk,
                                                 .capacity = capacity, .append = s != 0});
            if (r == MM_OK &&
                hipMemcpyAsync(&h[s + 1], ws->total, sizeof(unsigned long long), hipMemcpyDeviceToHost,
                               ws->stream) != hipSuccess)
                r = MM_ERR_HIP;
        }
        hipError_t e = hipMemcpyAsync(ws->h_total, ws->total, 2 * sizeof(unsigned long long),
                                      hipMemcpyDeviceToHost, ws->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ws->stream);
        if (r == MM_OK && e != hipSuccess) r = hip_fail(e, "batch sync");
        if (r == MM_OK) {
            out_offsets[0] = 0;
            for (uint64_t s = 0; s < n_seqs; ++s) out_offsets[s + 1] = h[s + 1];
        }
        hipHostFree(h);
        if (r) return r;
        const int je = judge_run_error(ws);
        if (je < 0) return je;
        if (je == 0) break;  // (1: redo the batch in ticket mode)
    }
    if (d_out_pos && out_offsets[n_seqs] > capacity) return MM_ERR_CAPACITY;
    return MM_OK;
}

// Batched short reads: read r = bases [base_offset + r * read_stride, + len_r) of one packed buffer.
// Fast path: the reads-mode fused kernel (one lane per read, one launch; prebuilt for minimizers,
// specialised at first use for the syncmer modes and other w).  Anything it cannot take (w > 128,
// reads too long for the LDS lists) runs one launch per read on the same stream: slower, same results.
static int run_reads_async_impl(const mm_plan_t *plan, mm_workspace_t *ws, const ReadsCall &c) {
    uint32_t *d_out_sk = c.d_out_sk;
    uint64_t capacity = c.capacity;
    if (!plan || !ws || !c.d_out_offsets) return MM_ERR_NULL;
    if (c.n_reads >= (1ull << 32)) return MM_ERR_LEN_TOO_LARGE;
    // (back-to-back reads WITH ambiguity bits: mm_run_packed_reads_skip_ambiguous_* - bit j of the span belongs to base j)
    if (c.d_read_starts && c.d_read_lens) return MM_ERR_BAD_MODE;
    if (c.amb && !plan->canonical_windows) return MM_ERR_HASHER_NOT_CANONICAL;
    if (d_out_sk && plan->mode != MM_MINIMIZERS) return MM_ERR_BAD_MODE;  // src/lib.rs:339
    if (d_out_sk && c.amb) return MM_ERR_BAD_MODE;  // the reference has no skip-ambiguous super-k-mer run
    if (!c.d_out_pos) {
        capacity = 0;
        d_out_sk = nullptr;
    }
    MM_HIP(set_device(ws->device));
    MM_HIP(hipMemsetAsync(ws->total, 0, 2 * sizeof(unsigned long long), ws->stream));
    if (c.n_reads == 0 || c.read_len == 0) {
        MM_HIP(hipMemsetAsync(c.d_out_offsets, 0, (c.n_reads + 1) * sizeof(uint64_t), ws->stream));
        if (c.d_count) MM_HIP(hipMemsetAsync(c.d_count, 0, sizeof(uint64_t), ws->stream));
        return MM_OK;
    }
    if (!c.d_packed) return MM_ERR_NULL;
    const uint64_t span = c.d_read_starts ? c.total_bases : (c.n_reads - 1) * (uint64_t)c.read_stride + c.read_len;
    if (span >= (1ull << 32)) return MM_ERR_LEN_TOO_LARGE;
    // bases of all reads together, which bound a lane table's lanes: reads back to back cover their span once, fixed-stride
    // reads may OVERLAP (read_len > read_stride: 5 kbp windows every 1 kbp) and then cover it several times
    const uint64_t read_bases = c.d_read_starts ? span : (span > c.n_reads * (uint64_t)c.read_len ? span : c.n_reads * (uint64_t)c.read_len);
    mm::SeqView view;
    int r = make_view(c.d_packed, c.packed_bytes, c.base_offset, span, &view);
    if (r) return r;

    bool fast = !ws->force_generic && mm::fused_reads_supported(plan->w, plan->canonical_windows, (int)plan->ht.canonical,
                                                                plan->mode, d_out_sk != nullptr);
    ws->last_lane_table = false;  // (also when no reads-mode kernel serves the plan: one launch per read below)
    if (fast) {
        mm::ReadsArgs a{};
        a.seq = view;
        set_packed_plan(a, plan);
        a.n_reads = c.n_reads;
        a.read_stride = c.read_stride;
        a.read_len = c.read_len;
        a.read_lens = c.d_read_lens;
        a.read_starts = reinterpret_cast<const unsigned long long *>(c.d_read_starts);
        a.read_offsets = reinterpret_cast<unsigned long long *>(c.d_out_offsets);
        a.out = out_params(ws, c.d_out_pos, d_out_sk, capacity);
        a.use_ticket = use_ticket(ws);
        const uint64_t l = (uint64_t)plan->k + plan->w - 1;
        if (c.amb && span >= l) {
            r = prepare_window_ambiguity(ws, *c.amb, span, (uint32_t)l, 0, span - l + 1, &a.wamb_dwords);
            if (r) return r;
            a.wamb = ws->wamb;
        }
        // One lane per read (rounds 2-5) while the longest read fits a default lane; the lane table (round 6) for
        // longer ones - a lane per read then needs lists that leave a CU one or two workgroups, and above about 1.5 kbp
        // none at all (the per-read loop below, 33 us per read, was what a HiFi / ONT batch got).
        const int policy = lane_table_policy();
        bool lanes = policy == 1;
        if (policy == -1) {
            // (one lane per read stays while its lists leave a CU three workgroups - 48 KB: 1.3 x density x windows + 8 entries
            // of 516 bytes - and never below the lane table's own lane length.  Measured on the ladder's rungs, k=21 w=11,
            // tools/gpu_reads_crossover.py, profiles/r06_reads_crossover.txt: reads of up to 353 windows 0.68 / 0.87 ms one lane
            // each against 0.79 / 1.00 through the table (forward / canonical); up to 481 windows 0.92 / 1.18 against 0.74 / 0.95)
            mm::SegPlan sp;
            const uint64_t max_nw = c.read_len >= l ? c.read_len - l + 1 : 0;
            const double dens = expected_density(plan);
            const uint64_t one_lane = (uint64_t)((48.0 * 1024.0 / 516.0 - 8.0) / (1.3 * dens));
            lanes = mm::fused_segments_plan(a, read_bases, ws->nblk, &sp) == 0 && max_nw > (sp.S > one_lane ? sp.S : one_lane);
        }
        int lr = -3;
        if (lanes) {
            const mm::SegSource src{a.read_starts, a.read_starts ? nullptr : c.d_read_lens, c.read_stride, c.read_len};
            r = run_lane_table(ws, a, src, read_bases);
            if (r < 0) return r;
            lr = r == 0 ? 0 : -3;
        }
        if (lr != 0) {
            r = grow_status(ws, mm::fused_reads_status_words(a));
            if (r) return r;
            a.out.status = ws->status;
            r = next_status_epoch(ws, &a.status_epoch);
            if (r) return r;
            TimedLaunch timed(ws);
            r = timed.arm(a);
            if (r) return r;
            lr = mm::launch_fused_reads(a, ws->stream);
            if (lr == 0) {
                timed.done(MM_PATH_FUSED);
            } else {
                if (lr == -1) return launch_failed();
                timed.drop();  // (a lane-table launch below times itself)
                // (reads too long for one lane each and no lane-table launch either - switched off, or no kernel)
                if (lr == -3 && !lanes && policy != 0) {
                    const mm::SegSource src{a.read_starts, a.read_starts ? nullptr : c.d_read_lens, c.read_stride, c.read_len};
                    r = run_lane_table(ws, a, src, read_bases);
                    if (r < 0) return r;
                    if (r == 0) lr = 0;
                }
                if (lr != 0) fast = false;
            }
        }
    }
    if (!fast) {
        std::vector<uint32_t> lens;
        std::vector<uint64_t> starts;
        if (c.d_read_starts) {
            starts.resize(c.n_reads + 1);
            MM_HIP(hipMemcpyAsync(starts.data(), c.d_read_starts, (c.n_reads + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost,
                                  ws->stream));
            MM_HIP(hipStreamSynchronize(ws->stream));
        }
        if (c.d_read_lens) {
            lens.resize(c.n_reads);
            MM_HIP(hipMemcpyAsync(lens.data(), c.d_read_lens, c.n_reads * sizeof(uint32_t),
                                  hipMemcpyDeviceToHost, ws->stream));
            MM_HIP(hipStreamSynchronize(ws->stream));
        }
        MM_HIP(hipMemsetAsync(c.d_out_offsets, 0, sizeof(uint64_t), ws->stream));
        const uint8_t *bytes = static_cast<const uint8_t *>(c.d_packed);
        for (uint64_t i = 0; i < c.n_reads; ++i) {
            const uint64_t first = c.base_offset + (c.d_read_starts ? starts[i] : i * (uint64_t)c.read_stride);
            uint64_t len = c.d_read_lens ? (lens[i] < c.read_len ? lens[i] : c.read_len) : c.read_len;
            if (c.d_read_starts) len = starts[i + 1] - starts[i] < c.read_len ? starts[i + 1] - starts[i] : c.read_len;
            AmbArgs ra;
            if (c.amb) ra = AmbArgs{c.amb->d_amb, c.amb->bytes, c.amb->bit_offset + (c.d_read_starts ? starts[i] : i * (uint64_t)c.read_stride)};
            r = run_device_async_impl(plan, ws, {.d_packed = bytes + first / 4, .packed_bytes = c.packed_bytes - first / 4,
                                                 .base_offset = first % 4, .n_bases = len, .win_end = UINT64_MAX,
                                                 .d_out_pos = c.d_out_pos, .d_out_sk = d_out_sk, .capacity = capacity,
                                                 .append = i != 0, .amb = c.amb ? &ra : nullptr});
            if (r) return r;
            MM_HIP(hipMemcpyAsync(c.d_out_offsets + i + 1, ws->total, sizeof(uint64_t),
                                  hipMemcpyDeviceToDevice, ws->stream));
        }
    }
    if (c.d_count)
        MM_HIP(hipMemcpyAsync(c.d_count, ws->total, sizeof(unsigned long long), hipMemcpyDeviceToDevice,
                              ws->stream));
    return MM_OK;
}

// (the call's d_count stays null: the count comes back through the workspace's host words)
static int run_reads_sync(const mm_plan_t *plan, mm_workspace_t *ws, const ReadsCall &c, uint64_t *out_count) {
    return run_sync(ws, c.capacity, c.d_out_pos != nullptr, out_count, [&](bool *) { return run_reads_async_impl(plan, ws, c); });
}

// Reads packed back to back (the FASTQ / FASTA packers' layout): read r = bases [d_read_starts[r], d_read_starts[r + 1]).
int mm_run_packed_reads_device_async(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed,
                                     uint64_t packed_bytes, uint64_t base_offset, uint64_t n_reads,
                                     const uint64_t *d_read_starts, uint64_t total_bases, uint32_t max_read_len,
                                     uint32_t *d_out_pos, uint32_t *d_out_sk, uint64_t capacity, uint64_t *d_out_offsets,
                                     uint64_t *d_count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (const int bad = dna_plan_only(plan)) return bad;
    if (!d_read_starts && n_reads) return MM_ERR_NULL;
    if (ws) ws->async_unchecked = true;
    return run_reads_async_impl(plan, ws, {.d_packed = d_packed, .packed_bytes = packed_bytes, .base_offset = base_offset,
                                           .n_reads = n_reads, .read_len = max_read_len, .d_read_starts = d_read_starts,
                                           .total_bases = total_bases, .d_out_pos = d_out_pos, .d_out_sk = d_out_sk,
                                           .capacity = capacity, .d_out_offsets = d_out_offsets, .d_count = d_count});
}

int mm_run_packed_reads_device(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed, uint64_t packed_bytes,
                               uint64_t base_offset, uint64_t n_reads, const uint64_t *d_read_starts, uint64_t total_bases,
                               uint32_t max_read_len, uint32_t *d_out_pos, uint32_t *d_out_sk, uint64_t capacity,
                               uint64_t *d_out_offsets, uint64_t *out_count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (const int bad = dna_plan_only(plan)) return bad;
    if (!ws || (!d_read_starts && n_reads)) return MM_ERR_NULL;
    return run_reads_sync(plan, ws, {.d_packed = d_packed, .packed_bytes = packed_bytes, .base_offset = base_offset,
                                     .n_reads = n_reads, .read_len = max_read_len, .d_read_starts = d_read_starts,
                                     .total_bases = total_bases, .d_out_pos = d_out_pos, .d_out_sk = d_out_sk,
                                     .capacity = capacity, .d_out_offsets = d_out_offsets}, out_count);
}

// Builder::run_skip_ambiguous_windows (src/lib.rs:451-496) per record of a back-to-back buffer: what the *_pack_n packers
// write goes straight in.  The refusals that need no device come first, the workspace last.
static int packed_reads_skip_check(const mm_plan_t *plan, const void *d_amb, uint64_t n_reads, const uint64_t *d_read_starts) {
    if (const int bad = dna_plan_only(plan)) return bad;
    if (plan && !plan->canonical_windows) return MM_ERR_HASHER_NOT_CANONICAL;
    if (n_reads && (!d_read_starts || !d_amb)) return MM_ERR_NULL;
    return MM_OK;
}

int mm_run_packed_reads_skip_ambiguous_device_async(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed,
                                                    uint64_t packed_bytes, uint64_t base_offset, const void *d_amb,
                                                    uint64_t amb_bytes, uint64_t amb_offset, uint64_t n_reads,
                                                    const uint64_t *d_read_starts, uint64_t total_bases,
                                                    uint32_t max_read_len, uint32_t *d_out_pos, uint64_t capacity,
                                                    uint64_t *d_out_offsets, uint64_t *d_count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    const int c = packed_reads_skip_check(plan, d_amb, n_reads, d_read_starts);
    if (c) return c;
    if (ws) ws->async_unchecked = true;
    const AmbArgs amb{d_amb, amb_bytes, amb_offset};
    return run_reads_async_impl(plan, ws, {.d_packed = d_packed, .packed_bytes = packed_bytes, .base_offset = base_offset,
                                           .n_reads = n_reads, .read_len = max_read_len, .d_read_starts = d_read_starts,
                                           .total_bases = total_bases, .d_out_pos = d_out_pos, .capacity = capacity,
                                           .d_out_offsets = d_out_offsets, .d_count = d_count, .amb = &amb});
}

int mm_run_packed_reads_skip_ambiguous_device(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed,
                                              uint64_t packed_bytes, uint64_t base_offset, const void *d_amb,
                                              uint64_t amb_bytes, uint64_t amb_offset, uint64_t n_reads,
                                              const uint64_t *d_read_starts, uint64_t total_bases,
                                              uint32_t max_read_len, uint32_t *d_out_pos, uint64_t capacity,
                                              uint64_t *d_out_offsets, uint64_t *out_count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    const int c = packed_reads_skip_check(plan, d_amb, n_reads, d_read_starts);
    if (c) return c;
    const AmbArgs amb{d_amb, amb_bytes, amb_offset};
    return run_reads_sync(plan, ws, {.d_packed = d_packed, .packed_bytes = packed_bytes, .base_offset = base_offset,
                                     .n_reads = n_reads, .read_len = max_read_len, .d_read_starts = d_read_starts,
                                     .total_bases = total_bases, .d_out_pos = d_out_pos, .capacity = capacity,
                                     .d_out_offsets = d_out_offsets, .amb = &amb}, out_count);
}

// --------------------------------------------- packed reads, counts on the device
// mm_run_packed_reads_device_async with its counts in DEVICE memory (d_counts, the layout mm_fastq_pack_device_async and
// mm_fasta_pack_device_async write: bases, records), read when the kernels run: packer and run queue back to back,
// nothing waits for the host.  The host knows upper bounds only and sizes the lane table, the walk's grid and the
// workspace buffers from them; the table kernels do the rest (mm_lane_counts.h, mm_lanes.hip).  The run ALWAYS takes the
// lane table: one lane per read needs max_read_len and n_reads inside the walk.  The reference has no counterpart
// (its loader and Builder::run are synchronous host code, bench/src/lib.rs:51-82, src/lib.rs:378); the results are those
// of mm_run_packed_reads_device_async given the counts as host arguments and max_read_len = 0xffffffff.
// The argument checks, before anything is touched, in the documented order; the workspace is looked at for
// mm_workspace_force_generic and the lane length only, and refused last when it is NULL.
static int packed_reads_counts_check(const mm_plan_t *plan, const mm_workspace_t *ws, const ReadsCountsCall &c) {
    if (!plan) return MM_ERR_NULL;
    if (plan->text) return MM_ERR_BAD_MODE;  // (a plan of mm_plan_create_text: text entry points only)
    if (c.max_bases >= (1ull << 32) || c.max_records >= (1ull << 31)) return MM_ERR_LEN_TOO_LARGE;
    if (c.d_out_sk && plan->mode != MM_MINIMIZERS) return MM_ERR_BAD_MODE;  // src/lib.rs:339
    if (c.amb && !plan->canonical_windows) return MM_ERR_HASHER_NOT_CANONICAL;  // src/lib.rs:451
    if (!c.d_out_offsets || !c.d_counts || !c.d_read_starts || !c.d_packed || (c.amb && !c.amb->d_amb)) return MM_ERR_NULL;
    if (c.base_offset > 4 * c.packed_bytes || c.max_bases > 4 * c.packed_bytes - c.base_offset) return MM_ERR_CAPACITY;
    if (c.amb && (c.amb->bit_offset > 8 * c.amb->bytes || c.max_bases > 8 * c.amb->bytes - c.amb->bit_offset)) return MM_ERR_CAPACITY;
    // a plan without a lane-table launch: the per-read paths need the counts on the host
    const char *why = nullptr;
    if (ws && ws->force_generic) why = "the generic family (mm_workspace_force_generic) runs one launch per read";
    else if (!mm::fused_reads_supported(plan->w, plan->canonical_windows, (int)plan->ht.canonical, plan->mode, c.d_out_sk != nullptr))
        why = "no reads-mode kernel for this plan (w > 128, or MM_JIT=0 and no prebuilt instance)";
    else if (lane_table_policy() == 0) why = "MM_LANE_TABLE=0 switches the lane table off";
    else {
        mm::ReadsArgs a{};
        set_plan(a, plan);  // (the planner asks for sizes only: no tables)
        a.n_reads = c.max_records ? c.max_records : 1;
        a.out.sk = const_cast<uint32_t *>(c.d_out_sk);
        a.wamb = c.amb ? reinterpret_cast<const uint32_t *>(c.amb->d_amb) : nullptr;  // (only "is there one" is asked)
        mm::SegPlan sp;
        if (mm::fused_segments_plan(a, c.max_bases, ws ? ws->nblk : 0u, &sp) != 0) why = "no lane length fits this plan";
    }
    if (why) {
        g_last_error = std::string("mm_run_packed_reads_counts_device*: ") + why +
                       "; read the counts back and call mm_run_packed_reads_device";
        return MM_ERR_BAD_MODE;
    }
    return ws ? MM_OK : MM_ERR_NULL;
}

static int run_reads_counts_async_impl(const mm_plan_t *plan, mm_workspace_t *ws, const ReadsCountsCall &c) {
    int r = packed_reads_counts_check(plan, ws, c);
    if (r) return r;
    const uint64_t max_bases = c.max_bases, max_records = c.max_records;
    const AmbArgs *const amb = c.amb;
    uint64_t *const d_count = c.d_count;
    MM_HIP(set_device(ws->device));
    mm::ReadsArgs a{};
    r = make_view(c.d_packed, c.packed_bytes, c.base_offset, max_bases, &a.seq);
    if (r) return r;
    set_packed_plan(a, plan);
    a.n_reads = max_records ? max_records : 1;  // (what sizes the launch; the walk is given max_records itself)
    a.read_len = 0xffffffffu;
    a.read_starts = reinterpret_cast<const unsigned long long *>(c.d_read_starts);
    a.read_offsets = reinterpret_cast<unsigned long long *>(c.d_out_offsets);
    // (no positions asked for: no capacity, no indices)
    a.out = out_params(ws, c.d_out_pos, c.d_out_pos ? c.d_out_sk : nullptr, c.d_out_pos ? c.capacity : 0);
    a.use_ticket = use_ticket(ws);
    MM_HIP(hipMemsetAsync(ws->total, 0, 2 * sizeof(unsigned long long), ws->stream));
    const uint64_t l = (uint64_t)plan->k + plan->w - 1;
    if (amb) {
        // the window bits of the whole BOUND span (the packers clear d_amb; a lane only reads window bits inside its
        // record).  A bound below l has no window: one cleared dword stands for the bits, so that the plan keeps its
        // landing area
        if (max_bases >= l) {
            r = prepare_window_ambiguity(ws, *amb, max_bases, (uint32_t)l, 0, max_bases - l + 1, &a.wamb_dwords);
            if (r) return r;
        } else {
            r = grow(ws->wamb, ws->wamb_dwords, 16, sizeof(uint32_t));
            if (r) return r;
            MM_HIP(hipMemsetAsync(ws->wamb, 0, 16 * sizeof(uint32_t), ws->stream));
            a.wamb_dwords = 16;
        }
        a.wamb = ws->wamb;
    }
    mm::SegSource src{a.read_starts, nullptr, 0, 0xffffffffu};
    src.counts = reinterpret_cast<const unsigned long long *>(c.d_counts);
    src.max_bases = (uint32_t)max_bases;
    src.max_records = (uint32_t)max_records;
    r = run_lane_table(ws, a, src, max_bases);
    if (r < 0) return r;
    if (r != 0) {  // (the check above found a lane-table launch for this plan: only a kernel that failed to compile ends here)
        g_last_error = std::string("mm_run_packed_reads_counts_device*: no reads-mode kernel (") + mm::fused_unavailable_reason() +
                       "); read the counts back and call mm_run_packed_reads_device";
        return MM_ERR_BAD_MODE;
    }
    if (d_count)
        MM_HIP(hipMemcpyAsync(d_count, ws->total, sizeof(unsigned long long), hipMemcpyDeviceToDevice, ws->stream));
    return MM_OK;
}

static int run_reads_counts_sync(const mm_plan_t *plan, mm_workspace_t *ws, const ReadsCountsCall &c, uint64_t *out) {
    const int rc = packed_reads_counts_check(plan, ws, c);
    if (rc) return rc;
    return run_counts_sync(ws, c.d_counts, c.capacity, c.d_out_pos != nullptr, out,
                           [&]() { return run_reads_counts_async_impl(plan, ws, c); });
}

int mm_run_packed_reads_counts_device_async(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed,
                                            uint64_t packed_bytes, uint64_t base_offset, uint64_t max_bases,
                                            uint64_t max_records, const uint64_t *d_read_starts, const uint64_t *d_counts,
                                            uint32_t *d_out_pos, uint32_t *d_out_sk, uint64_t capacity,
                                            uint64_t *d_out_offsets, uint64_t *d_count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (ws) ws->async_unchecked = true;
    return run_reads_counts_async_impl(plan, ws, {.d_packed = d_packed, .packed_bytes = packed_bytes, .base_offset = base_offset,
                                                  .max_bases = max_bases, .max_records = max_records,
                                                  .d_read_starts = d_read_starts, .d_counts = d_counts, .d_out_pos = d_out_pos,
                                                  .d_out_sk = d_out_sk, .capacity = capacity, .d_out_offsets = d_out_offsets,
                                                  .d_count = d_count});
}

int mm_run_packed_reads_counts_device(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed, uint64_t packed_bytes,
                                      uint64_t base_offset, uint64_t max_bases, uint64_t max_records,
                                      const uint64_t *d_read_starts, const uint64_t *d_counts, uint32_t *d_out_pos,
                                      uint32_t *d_out_sk, uint64_t capacity, uint64_t *d_out_offsets, uint64_t *out) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    return run_reads_counts_sync(plan, ws, {.d_packed = d_packed, .packed_bytes = packed_bytes, .base_offset = base_offset,
                                            .max_bases = max_bases, .max_records = max_records, .d_read_starts = d_read_starts,
                                            .d_counts = d_counts, .d_out_pos = d_out_pos, .d_out_sk = d_out_sk,
                                            .capacity = capacity, .d_out_offsets = d_out_offsets}, out);
}

// Builder::run_skip_ambiguous_windows (src/lib.rs:451-496) per record with the counts on the device: what the *_pack_n
// packers write goes straight in, on the packer's stream.
int mm_run_packed_reads_skip_ambiguous_counts_device_async(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed,
                                                           uint64_t packed_bytes, uint64_t base_offset, const void *d_amb,
                                                           uint64_t amb_bytes, uint64_t amb_offset, uint64_t max_bases,
                                                           uint64_t max_records, const uint64_t *d_read_starts,
                                                           const uint64_t *d_counts, uint32_t *d_out_pos, uint64_t capacity,
                                                           uint64_t *d_out_offsets, uint64_t *d_count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (ws) ws->async_unchecked = true;
    const AmbArgs amb{d_amb, amb_bytes, amb_offset};
    return run_reads_counts_async_impl(plan, ws, {.d_packed = d_packed, .packed_bytes = packed_bytes, .base_offset = base_offset,
                                                  .max_bases = max_bases, .max_records = max_records,
                                                  .d_read_starts = d_read_starts, .d_counts = d_counts, .d_out_pos = d_out_pos,
                                                  .capacity = capacity, .d_out_offsets = d_out_offsets, .d_count = d_count,
                                                  .amb = &amb});
}

int mm_run_packed_reads_skip_ambiguous_counts_device(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed,
                                                     uint64_t packed_bytes, uint64_t base_offset, const void *d_amb,
                                                     uint64_t amb_bytes, uint64_t amb_offset, uint64_t max_bases,
                                                     uint64_t max_records, const uint64_t *d_read_starts,
                                                     const uint64_t *d_counts, uint32_t *d_out_pos, uint64_t capacity,
                                                     uint64_t *d_out_offsets, uint64_t *out) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    const AmbArgs amb{d_amb, amb_bytes, amb_offset};
    return run_reads_counts_sync(plan, ws, {.d_packed = d_packed, .packed_bytes = packed_bytes, .base_offset = base_offset,
                                            .max_bases = max_bases, .max_records = max_records, .d_read_starts = d_read_starts,
                                            .d_counts = d_counts, .d_out_pos = d_out_pos, .capacity = capacity,
                                            .d_out_offsets = d_out_offsets, .amb = &amb}, out);
}

// What the table kernels of the counts calls make of {counts, bounds}, by the function they call (mm_lane_counts.h): no device.
int mm_debug_lane_counts_view(uint64_t max_bases, uint64_t max_records, uint64_t n_bases, uint64_t n_records, uint64_t out[3]) {
    if (!out) return MM_ERR_NULL;
    if (max_bases >= (1ull << 32) || max_records >= (1ull << 31)) return MM_ERR_LEN_TOO_LARGE;  // (the entry points' rule)
    const mm::LaneCountsView v = mm::lane_counts_view(max_bases, max_records, n_bases, n_records);
    out[0] = v.n_reads_eff;
    out[1] = v.refused;
    out[2] = mm::lane_counts_bound(max_bases, max_records, 1u);
    return MM_OK;
}

int mm_run_reads_device_async(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed,
                              uint64_t packed_bytes, uint64_t base_offset, uint64_t n_reads,
                              uint32_t read_stride, uint32_t read_len, const uint32_t *d_read_lens,
                              uint32_t *d_out_pos, uint64_t capacity, uint64_t *d_out_offsets,
                              uint64_t *d_count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (const int bad = dna_plan_only(plan)) return bad;
    if (ws) ws->async_unchecked = true;
    return run_reads_async_impl(plan, ws, {.d_packed = d_packed, .packed_bytes = packed_bytes, .base_offset = base_offset,
                                           .n_reads = n_reads, .read_stride = read_stride, .read_len = read_len,
                                           .d_read_lens = d_read_lens, .d_out_pos = d_out_pos, .capacity = capacity,
                                           .d_out_offsets = d_out_offsets, .d_count = d_count});
}

int mm_run_reads_device(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed,
                        uint64_t packed_bytes, uint64_t base_offset, uint64_t n_reads,
                        uint32_t read_stride, uint32_t read_len, const uint32_t *d_read_lens,
                        uint32_t *d_out_pos, uint64_t capacity, uint64_t *d_out_offsets,
                        uint64_t *out_count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (const int bad = dna_plan_only(plan)) return bad;
    return run_reads_sync(plan, ws, {.d_packed = d_packed, .packed_bytes = packed_bytes, .base_offset = base_offset,
                                     .n_reads = n_reads, .read_stride = read_stride, .read_len = read_len,
                                     .d_read_lens = d_read_lens, .d_out_pos = d_out_pos, .capacity = capacity,
                                     .d_out_offsets = d_out_offsets}, out_count);
}

int mm_run_reads_superkmers_device_async(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed,
                                         uint64_t packed_bytes, uint64_t base_offset, uint64_t n_reads,
                                         uint32_t read_stride, uint32_t read_len, const uint32_t *d_read_lens,
                                         uint32_t *d_out_pos, uint32_t *d_out_sk, uint64_t capacity,
                                         uint64_t *d_out_offsets, uint64_t *d_count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (const int bad = dna_plan_only(plan)) return bad;
    if (ws) ws->async_unchecked = true;
    if (!d_out_sk) return MM_ERR_NULL;
    return run_reads_async_impl(plan, ws, {.d_packed = d_packed, .packed_bytes = packed_bytes, .base_offset = base_offset,
                                           .n_reads = n_reads, .read_stride = read_stride, .read_len = read_len,
                                           .d_read_lens = d_read_lens, .d_out_pos = d_out_pos, .d_out_sk = d_out_sk,
                                           .capacity = capacity, .d_out_offsets = d_out_offsets, .d_count = d_count});
}

int mm_run_reads_superkmers_device(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed,
                                   uint64_t packed_bytes, uint64_t base_offset, uint64_t n_reads,
                                   uint32_t read_stride, uint32_t read_len, const uint32_t *d_read_lens,
                                   uint32_t *d_out_pos, uint32_t *d_out_sk, uint64_t capacity,
                                   uint64_t *d_out_offsets, uint64_t *out_count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (const int bad = dna_plan_only(plan)) return bad;
    if (!d_out_sk) return MM_ERR_NULL;
    return run_reads_sync(plan, ws, {.d_packed = d_packed, .packed_bytes = packed_bytes, .base_offset = base_offset,
                                     .n_reads = n_reads, .read_stride = read_stride, .read_len = read_len,
                                     .d_read_lens = d_read_lens, .d_out_pos = d_out_pos, .d_out_sk = d_out_sk,
                                     .capacity = capacity, .d_out_offsets = d_out_offsets}, out_count);
}

int mm_run_reads_skip_ambiguous_device_async(const mm_plan_t *plan, mm_workspace_t *ws,
                                             const void *d_packed, uint64_t packed_bytes,
                                             uint64_t base_offset, const void *d_amb, uint64_t amb_bytes,
                                             uint64_t amb_offset, uint64_t n_reads, uint32_t read_stride,
                                             uint32_t read_len, const uint32_t *d_read_lens,
                                             uint32_t *d_out_pos, uint64_t capacity,
                                             uint64_t *d_out_offsets, uint64_t *d_count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (const int bad = dna_plan_only(plan)) return bad;
    if (ws) ws->async_unchecked = true;
    const AmbArgs amb{d_amb, amb_bytes, amb_offset};
    return run_reads_async_impl(plan, ws, {.d_packed = d_packed, .packed_bytes = packed_bytes, .base_offset = base_offset,
                                           .n_reads = n_reads, .read_stride = read_stride, .read_len = read_len,
                                           .d_read_lens = d_read_lens, .d_out_pos = d_out_pos, .capacity = capacity,
                                           .d_out_offsets = d_out_offsets, .d_count = d_count, .amb = &amb});
}

int mm_run_reads_skip_ambiguous_device(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed,
                                       uint64_t packed_bytes, uint64_t base_offset, const void *d_amb,
                                       uint64_t amb_bytes, uint64_t amb_offset, uint64_t n_reads,
                                       uint32_t read_stride, uint32_t read_len,
                                       const uint32_t *d_read_lens, uint32_t *d_out_pos,
                                       uint64_t capacity, uint64_t *d_out_offsets, uint64_t *out_count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (const int bad = dna_plan_only(plan)) return bad;
    const AmbArgs amb{d_amb, amb_bytes, amb_offset};
    return run_reads_sync(plan, ws, {.d_packed = d_packed, .packed_bytes = packed_bytes, .base_offset = base_offset,
                                     .n_reads = n_reads, .read_stride = read_stride, .read_len = read_len,
                                     .d_read_lens = d_read_lens, .d_out_pos = d_out_pos, .capacity = capacity,
                                     .d_out_offsets = d_out_offsets, .amb = &amb}, out_count);
}

// ---- PackedNSeq: Builder::run_skip_ambiguous_windows (src/lib.rs:451-496)
int mm_run_skip_ambiguous_device_async(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed,
                                       uint64_t packed_bytes, uint64_t base_offset, const void *d_amb,
                                       uint64_t amb_bytes, uint64_t amb_offset, uint64_t n_bases,
                                       uint64_t win_begin, uint64_t win_end, uint32_t *d_out_pos,
                                       uint64_t capacity, uint64_t *d_count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (const int bad = dna_plan_only(plan)) return bad;
    if (ws) ws->async_unchecked = true;
    const AmbArgs amb{d_amb, amb_bytes, amb_offset};
    return run_device_async_impl(plan, ws, {.d_packed = d_packed, .packed_bytes = packed_bytes, .base_offset = base_offset,
                                            .n_bases = n_bases, .win_begin = win_begin, .win_end = win_end,
                                            .d_out_pos = d_out_pos, .capacity = capacity, .d_count = d_count, .amb = &amb});
}

// (the call's d_count, append and host words are not the caller's to set here)
static int run_device_sync(const mm_plan_t *plan, mm_workspace_t *ws, const SeqCall &c, uint64_t *out_count) {
    // One stream operation per call when the fused kernel runs: its last tile stores the total straight into the
    // page-locked word h_total[0] and a tile that raises an error stores the code into h_total[1] (flag_error),
    // so the host only waits for the stream.  (Rounds 1-3: two clears, the kernel, a copy - about 33 us a call.)
    // The split path, the generic family and empty runs leave host_written false: the device words, cleared by the
    // run itself, are copied.
    return run_sync(ws, c.capacity, c.d_out_pos != nullptr, out_count, [&](bool *host_written) -> int {
        ws->h_total[0] = 0;
        ws->h_total[1] = 0;
        // (no mapped host words on this runtime: the device's error word is read back, so clear it first)
        if (!ws->h_total_dev) MM_HIP(hipMemsetAsync(ws->total + 1, 0, sizeof(unsigned long long), ws->stream));
        SeqCall run = c;
        run.host_total_written = host_written;
        return run_device_async_impl(plan, ws, run);
    });
}

int mm_run_skip_ambiguous_device(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed,
                                 uint64_t packed_bytes, uint64_t base_offset, const void *d_amb,
                                 uint64_t amb_bytes, uint64_t amb_offset, uint64_t n_bases,
                                 uint64_t win_begin, uint64_t win_end, uint32_t *d_out_pos,
                                 uint64_t capacity, uint64_t *out_count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (const int bad = dna_plan_only(plan)) return bad;
    const AmbArgs amb{d_amb, amb_bytes, amb_offset};
    return run_device_sync(plan, ws, {.d_packed = d_packed, .packed_bytes = packed_bytes, .base_offset = base_offset,
                                      .n_bases = n_bases, .win_begin = win_begin, .win_end = win_end, .d_out_pos = d_out_pos,
                                      .capacity = capacity, .amb = &amb}, out_count);
}

int mm_run_device(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed,
                  uint64_t packed_bytes, uint64_t base_offset, uint64_t n_bases,
                  uint64_t win_begin, uint64_t win_end, uint32_t *d_out_pos, uint32_t *d_out_sk,
                  uint64_t capacity, uint64_t *out_count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (const int bad = dna_plan_only(plan)) return bad;
    return run_device_sync(plan, ws, {.d_packed = d_packed, .packed_bytes = packed_bytes, .base_offset = base_offset,
                                      .n_bases = n_bases, .win_begin = win_begin, .win_end = win_end, .d_out_pos = d_out_pos,
                                      .d_out_sk = d_out_sk, .capacity = capacity}, out_count);
}

// What a host entry point asks for: the sequence (packed bytes on the host, or already staged on the device) and the
// caller's HOST buffers for positions, indices and the count.
struct HostCall {
    const void *packed;
    uint64_t packed_bytes, base_offset, n_bases;
    uint32_t *out_pos, *out_sk;
    uint64_t capacity;
    uint64_t *out_count;
};

// (c.packed: the staged bytes on the device)
static int run_host_common(const mm_plan_t *plan, mm_workspace_t *ws, const HostCall &c, const AmbArgs *amb) {
    const uint64_t l = (uint64_t)plan->k + plan->w - 1;
    const uint64_t n_w = c.n_bases >= l ? c.n_bases - l + 1 : 0;
    const uint64_t cap = capped(c.out_pos, c.capacity, n_w);
    int r = stage_outputs(ws, cap, c.out_sk != nullptr);
    if (r) return r;
    uint64_t count = 0;
    r = run_device_sync(plan, ws, {.d_packed = c.packed, .packed_bytes = c.packed_bytes, .base_offset = c.base_offset,
                                   .n_bases = c.n_bases, .win_end = UINT64_MAX, .d_out_pos = cap ? ws->d_out : nullptr,
                                   .d_out_sk = (c.out_sk && cap) ? ws->d_sk : nullptr, .capacity = cap, .amb = amb}, &count);
    if (c.out_count) *c.out_count = count;
    if (r) return r;
    return download_positions(ws, c.out_pos, c.out_sk, count, nullptr, 0);
}

// Host entry point for long sequences, pipelined: the window range is cut into chunks; while chunk c is computed,
// the bytes of the chunks behind it travel host -> device and the positions of the chunks before it device -> host
// (the link is full duplex; the kernel itself is ~4 % of the call).
//
// Round 5.  The first version waited for chunk c - 1's kernel on the host (an event), read its
// total from a 16-byte device -> host copy queued on the kernel's stream, and only then queued that chunk's
// device -> host copy and the NEXT chunk's upload and kernel.  The trace of a call (profiles/r05_host_path.txt) showed
// what that costs: the 16-byte copy goes through the same copy engine as the 129 MB position copies and waits behind
// them, the next kernel waits behind IT in stream order, and the host wakes up once per chunk - uploads 2.5 ms apart
// instead of back to back.  Now the whole call is queued at once: all uploads, all kernels (each stores its running
// total into a page-locked word of its own: no copies on the kernels' stream), and the host only polls those words to
// size each chunk's device -> host copy, which waits for its kernel through an event on the device side.
// The mechanisms of the two legs can be switched (results identical; A/B per box, tools/host_link_diag.sh):
//   MM_HOST_OUT=blit (default: a copy kernel that reads its range from device memory and stores into the caller's
//   page-locked buffer - no host involvement, and no dependence on the state of the copy engines, see below) | engine
//   (hipMemcpyAsync) | direct (the fused kernel's own copy-out stores go straight into the caller's page-locked buffer);
//   MM_HOST_IN=engine (default) | blit;  MM_PIPE_CHUNKS=n.
// blit / direct need buffers the device can address (mm_host_alloc, hipHostMalloc, hipHostRegister); other buffers
// keep the engines.  Returns MM_PIPE_FALLBACK if the caller should take the one-shot path instead.
static const int MM_PIPE_FALLBACK = 1;
static const uint64_t kPipeMinWindows = 48ull << 20;
static const int kPipeMaxChunks = 64;
static const unsigned long long kPipeUnset = ~0ull;

// the device's address of page-locked host memory, or null (pageable memory, or the runtime does not say)
static void *device_alias_of_host(const void *p) {
    if (!p) return nullptr;
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    if (at.type != hipMemoryTypeHost || !at.devicePointer) return nullptr;
    return at.devicePointer;
}

static int run_host_pipelined(const mm_plan_t *plan, mm_workspace_t *ws, const HostCall &call) {
    const uint8_t *const packed = static_cast<const uint8_t *>(call.packed);
    const uint64_t base_offset = call.base_offset, n_bases = call.n_bases, capacity = call.capacity;
    uint32_t *const out_pos = call.out_pos, *const out_sk = call.out_sk;
    uint64_t *const out_count = call.out_count;
    const uint64_t l = (uint64_t)plan->k + plan->w - 1;
    const uint64_t n_w = n_bases >= l ? n_bases - l + 1 : 0;
    if (!out_pos || n_w < kPipeMinWindows || mm::mm_env("MM_NO_PIPELINE") || !ws->h_total_dev) return MM_PIPE_FALLBACK;
    const uint64_t cap = capacity < n_w ? capacity : n_w;
    if (cap == 0) return MM_PIPE_FALLBACK;
    const uint64_t bytes = (base_offset + n_bases + 3) / 4;
    if (!ws->copy_in) {
        MM_HIP(hipStreamCreateWithFlags(&ws->copy_in, hipStreamNonBlocking));
        MM_HIP(hipStreamCreateWithFlags(&ws->copy_out, hipStreamNonBlocking));
        for (int i = 0; i < kPipeMaxChunks; ++i) {
            MM_HIP(hipEventCreateWithFlags(&ws->ev_in[i], hipEventDisableTiming));
            MM_HIP(hipEventCreateWithFlags(&ws->ev_k[i], hipEventDisableTiming));
            MM_HIP(hipEventCreateWithFlags(&ws->ev_out[i], hipEventDisableTiming));
        }
        MM_HIP(hipHostMalloc(reinterpret_cast<void **>(&ws->h_pipe), kPipeMaxChunks * sizeof(unsigned long long),
                             hipHostMallocMapped | hipHostMallocCoherent));
        void *dp = nullptr;
        if (hipHostGetDevicePointer(&dp, ws->h_pipe, 0) != hipSuccess) {
            (void)hipGetLastError();
            dp = nullptr;
        }
        ws->h_pipe_dev = reinterpret_cast<unsigned long long *>(dp);
        MM_HIP(hipMalloc(reinterpret_cast<void **>(&ws->d_pipe), (kPipeMaxChunks + 1) * sizeof(unsigned long long)));
    }
    if (!ws->h_pipe_dev) return MM_PIPE_FALLBACK;
    // mechanisms of the two legs
    // Default since late round 5: uploads by a copy engine, downloads by the copy KERNEL.  The engines are 6 % faster once
    // they run at their rate (41.0 against 43.5 ms per call) - but a process whose link has been idle gets there only
    // after two to five calls: 68 / 48 / 39.5 ms in a fresh process, 91 / 78 / 71 / 71 / 71 / 44 / 41 ms at the end of
    // bench.py, with a 20 ms stall of the first copies in the trace - and a caller that makes one call now and then
    // lives in that state.  The copy kernel reads 43.5 ms from the second call on, every time
    // (profiles/r05_host_path.txt, tools/gpu_host_cold.py).  MM_HOST_OUT=engine selects the engines for downloads.
    int out_mode = 1, in_mode = 0;  // 0 engine, 1 blit kernel, 2 (out only) the fused kernel's own stores
    if (const char *e = mm::mm_env("MM_HOST_OUT")) out_mode = !strcmp(e, "blit") ? 1 : (!strcmp(e, "direct") ? 2 : 0);
    if (const char *e = mm::mm_env("MM_HOST_IN")) in_mode = !strcmp(e, "blit") ? 1 : 0;
    uint32_t *pos_alias = nullptr, *sk_alias = nullptr;
    if (out_mode) {
        pos_alias = static_cast<uint32_t *>(device_alias_of_host(out_pos));
        sk_alias = out_sk ? static_cast<uint32_t *>(device_alias_of_host(out_sk)) : nullptr;
        if (!pos_alias || (out_sk && !sk_alias)) out_mode = 0;
    }
    const uint8_t *in_alias = nullptr;
    if (in_mode) {
        in_alias = static_cast<const uint8_t *>(device_alias_of_host(packed));
        if (!in_alias || (reinterpret_cast<uintptr_t>(in_alias) & 15u)) in_mode = 0;
    }
    int r = MM_OK;
    if (out_mode != 2) {
        r = grow(ws->d_out, ws->d_out_elems, cap, sizeof(uint32_t));
        if (r == MM_OK && out_sk) r = grow(ws->d_sk, ws->d_sk_elems, cap, sizeof(uint32_t));
        if (r) return r;
    }
    uint32_t *const k_pos = out_mode == 2 ? pos_alias : ws->d_out;
    uint32_t *const k_sk = out_sk ? (out_mode == 2 ? sk_alias : ws->d_sk) : nullptr;
    uint64_t n_chunks = n_w / (24ull << 20);
    if (n_chunks > 16) n_chunks = 16;
    if (const char *e = mm::mm_env("MM_PIPE_CHUNKS")) n_chunks = (uint64_t)atoi(e);
    if (n_chunks < 2) n_chunks = 2;
    if (n_chunks > (uint64_t)kPipeMaxChunks) n_chunks = kPipeMaxChunks;
    const uint64_t chunk = (n_w + n_chunks - 1) / n_chunks;
    n_chunks = (n_w + chunk - 1) / chunk;
    uint8_t *din = reinterpret_cast<uint8_t *>(ws->d_in);
    const uint32_t kCopyWorkgroups = 64;

    // the per-run error word: raised by any chunk's kernel (flag_error stores the code into the page-locked word
    // too), read once at the end.  An *_async run still in flight on this stream would raise it into the same word.
    if (ws->async_unchecked) MM_HIP(hipStreamSynchronize(ws->stream));
    ws->h_total[1] = 0;
    for (uint64_t c = 0; c < n_chunks; ++c) ws->h_pipe[c] = kPipeUnset;
    if (out_mode == 1) MM_HIP(hipMemsetAsync(ws->d_pipe, 0, sizeof(unsigned long long), ws->stream));  // (range of chunk 0 starts at 0)

    // One host loop drives the call.  It queues uploads + kernels ahead (each kernel waits for its upload through an
    // event on the device side and stores its running total into its own page-locked word), polls those words, and
    // queues every chunk's device -> host copy the moment its size is known (the copy waits for its kernel on the
    // device side).  ENGINE copies are throttled: at most `lim_in` uploads and `lim_out` downloads are in the runtime's
    // hands at any time.  Measured (profiles/r05_host_path.txt): with all 16 uploads queued at once the call takes
    // 49.6 ms - the sum of the two directions, no overlap at all - and 75 ms with 32 or 64, against 40.1 ms with 8; the
    // runtime picks a copy engine per copy when it is QUEUED, queued uploads occupy engines while they wait for one
    // another in stream order, and the downloads then land behind them.  A copy KERNEL has no such arbitration.
    uint64_t lim_in = 2, lim_out = 2;
    if (const char *e = mm::mm_env("MM_PIPE_IN_FLIGHT")) lim_in = (uint64_t)atoi(e);
    if (const char *e = mm::mm_env("MM_PIPE_OUT_FLIGHT")) lim_out = (uint64_t)atoi(e);
    if (in_mode == 1) lim_in = 0;    // (copy kernels: queue everything)
    if (out_mode != 0) lim_out = 0;
    uint64_t sent = 0;  // bytes already on their way to the device
    auto submit_chunk = [&](uint64_t c) -> int {
        const uint64_t wb = c * chunk, we = (wb + chunk < n_w) ? wb + chunk : n_w;
        // bytes that hold the bases of windows < we (the last one ends at base we + l - 2), in whole 16-byte units
        uint64_t need = ((base_offset + we + l - 2) / 4 + 1 + 15) & ~15ull;
        if (need > bytes || we == n_w) need = bytes;
        if (need > sent) {
            if (in_mode == 1 && (need - sent) >= 16) {
                const uint64_t n16 = (need - sent) / 16;  // (sent stays a multiple of 16 until the last chunk)
                if (mm::launch_copy16(in_alias + sent, din + sent, n16, kCopyWorkgroups, ws->copy_in))
                    return hip_fail(hipGetLastError(), "copy16");
                if ((need - sent) % 16)
                    MM_HIP(hipMemcpyAsync(din + sent + 16 * n16, packed + sent + 16 * n16, (need - sent) % 16,
                                          hipMemcpyHostToDevice, ws->copy_in));
            } else {
                MM_HIP(hipMemcpyAsync(din + sent, packed + sent, need - sent, hipMemcpyHostToDevice, ws->copy_in));
            }
            sent = need;
        }
        MM_HIP(hipEventRecord(ws->ev_in[c], ws->copy_in));
        MM_HIP(hipStreamWaitEvent(ws->stream, ws->ev_in[c], 0));
        bool hw = false;
        const int rr = run_device_async_impl(
            plan, ws, {.d_packed = ws->d_in, .packed_bytes = bytes + 16, .base_offset = base_offset, .n_bases = n_bases,
                       .win_begin = wb, .win_end = we, .d_out_pos = k_pos, .d_out_sk = k_sk, .capacity = cap,
                       .d_count = out_mode == 1 ? reinterpret_cast<uint64_t *>(ws->d_pipe + c + 1) : nullptr, .append = c != 0,
                       .host_total_written = &hw, .host_word_dev = ws->h_pipe_dev + c});
        if (rr) return rr;
        // (families whose kernels do not store the total themselves: the device word, copied)
        if (!hw)
            MM_HIP(hipMemcpyAsync(&ws->h_pipe[c], ws->total, sizeof(unsigned long long), hipMemcpyDeviceToHost, ws->stream));
        MM_HIP(hipEventRecord(ws->ev_k[c], ws->stream));
        if (out_mode == 1) {
            MM_HIP(hipStreamWaitEvent(ws->copy_out, ws->ev_k[c], 0));
            if (mm::launch_copy_range(ws->d_out, pos_alias, ws->d_pipe + c, cap, kCopyWorkgroups, ws->copy_out) ||
                (out_sk && mm::launch_copy_range(ws->d_sk, sk_alias, ws->d_pipe + c, cap, kCopyWorkgroups, ws->copy_out)))
                return hip_fail(hipGetLastError(), "copy_range");
        }
        return MM_OK;
    };
    auto done = [&](hipEvent_t ev, bool *yes) -> int {
        const hipError_t q = hipEventQuery(ev);
        *yes = q == hipSuccess;
        if (q != hipSuccess && q != hipErrorNotReady) return hip_fail(q, "hipEventQuery");
        if (q != hipSuccess) (void)hipGetLastError();
        return MM_OK;
    };
    // MM_PIPE_TRACE=1 (diagnostics): host time stamps of every chunk's milestones, printed to stderr when the call ends
    struct ChunkTrace {
        double submit = 0, in_done = 0, count = 0, out_queued = 0, out_done = 0;
    };
    const bool tracing = mm::mm_env("MM_PIPE_TRACE") != nullptr;
    std::vector<ChunkTrace> tr(tracing ? n_chunks : 0);
    const auto t_call = std::chrono::steady_clock::now();
    auto now_ms = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count(); };
    uint64_t next_in = 0, in_retired = 0;    // chunks submitted / whose upload is known to be complete
    uint64_t next_out = 0, out_retired = 0;  // chunks whose count was taken / whose download is known to be complete
    uint64_t done_total = 0;
    bool over = false, broken = false;
    uint32_t idle = 0;
    // (the loop queues uploads, kernels and copy kernels that store into the CALLER's buffers; whatever
    // ends it - a refused launch, a failed query or copy - the call must not return while any of that is still in flight,
    // or a caller that frees its buffers on the error meets a device that still reads and writes them.  The loop's own
    // result is therefore collected first, the three streams are waited for whatever it says, then it is judged.)
    const int loop_rc = [&]() -> int {
    while (next_out < n_chunks && !broken) {
        bool progress = false;
        while (next_in < n_chunks && (lim_in == 0 || next_in - in_retired < lim_in)) {
            if (tracing) tr[next_in].submit = now_ms();
            r = submit_chunk(next_in++);
            if (r) return r;
            progress = true;
        }
        bool yes = false;
        if (lim_in && in_retired < next_in) {
            r = done(ws->ev_in[in_retired], &yes);
            if (r) return r;
            if (yes) {
                if (tracing) tr[in_retired].in_done = now_ms();
                ++in_retired, progress = true;
            }
        }
        if (lim_out && out_retired < next_out) {
            r = done(ws->ev_out[out_retired], &yes);
            if (r) return r;
            if (yes) {
                if (tracing) tr[out_retired].out_done = now_ms();
                ++out_retired, progress = true;
            }
        }
        if (next_out < next_in && (lim_out == 0 || next_out - out_retired < lim_out)) {
            const uint64_t c = next_out;
            volatile unsigned long long *word = ws->h_pipe + c;
            unsigned long long tot = *word;
            if (tot == kPipeUnset && (++idle & 255u) == 0u) {
                r = done(ws->ev_k[c], &yes);
                if (r) return r;
                if (yes) {  // the kernel is done: the word is final
                    tot = *word;
                    if (tot == kPipeUnset) broken = true;  // (no kernel stored it - a failed launch the error word names)
                }
            }
            if (tot != kPipeUnset) {
                if (tot < done_total) {
                    broken = true;
                } else {
                    if (tot > cap) over = true;
                    const uint64_t upto = tot < cap ? tot : cap;
                    if (tracing) tr[c].count = now_ms();
                    if (out_mode == 0 && upto > done_total) {
                        MM_HIP(hipStreamWaitEvent(ws->copy_out, ws->ev_k[c], 0));
                        MM_HIP(hipMemcpyAsync(out_pos + done_total, ws->d_out + done_total,
                                              (upto - done_total) * sizeof(uint32_t), hipMemcpyDeviceToHost, ws->copy_out));
                        if (out_sk)
                            MM_HIP(hipMemcpyAsync(out_sk + done_total, ws->d_sk + done_total,
                                                  (upto - done_total) * sizeof(uint32_t), hipMemcpyDeviceToHost, ws->copy_out));
                    }
                    if (lim_out) MM_HIP(hipEventRecord(ws->ev_out[c], ws->copy_out));
                    if (tracing) tr[c].out_queued = now_ms();
                    done_total = tot;
                    ++next_out;
                    progress = true;
                }
            }
        }
        if (!progress) __builtin_ia32_pause();
    }
    return MM_OK;
    }();
    {
        const hipError_t e0 = hipStreamSynchronize(ws->stream), e1 = hipStreamSynchronize(ws->copy_in),
                         e2 = hipStreamSynchronize(ws->copy_out);
        if (loop_rc) {
            (void)hipGetLastError();
            (void)judge_run_error(ws);  // (consumes the error words a chunk's kernel may have raised: the next call starts clean)
            return loop_rc;
        }
        if (e0 != hipSuccess) return hip_fail(e0, "hipStreamSynchronize");
        if (e1 != hipSuccess) return hip_fail(e1, "hipStreamSynchronize");
        if (e2 != hipSuccess) return hip_fail(e2, "hipStreamSynchronize");
    }
    if (tracing) {
        fprintf(stderr, "[mm pipe] %llu chunks, out=%d in=%d, in flight %llu / %llu, call %.2f ms\n", (unsigned long long)n_chunks,
                out_mode, in_mode, (unsigned long long)lim_in, (unsigned long long)lim_out, now_ms());
        for (uint64_t c = 0; c < n_chunks; ++c)
            fprintf(stderr, "[mm pipe]  chunk %2llu: queued %7.2f  upload done %7.2f  count known %7.2f  download queued %7.2f  done %7.2f\n",
                    (unsigned long long)c, tr[c].submit, tr[c].in_done, tr[c].count, tr[c].out_queued, tr[c].out_done);
    }
    const int je = judge_run_error(ws);
    if (je < 0) return je;
    if (je == 1) return MM_PIPE_FALLBACK;  // a look-back spin ran out in some chunk: the whole call again, one shot, ticket mode
    if (broken) {
        g_last_error = "mm_run_host: a chunk's kernel finished without storing its count";
        return MM_ERR_HIP;
    }
    if (out_count) *out_count = done_total;
    return over || done_total > capacity ? MM_ERR_CAPACITY : MM_OK;
}

int mm_host_alloc(void **out, uint64_t bytes) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!out) return MM_ERR_NULL;
    *out = nullptr;
    if (bytes == 0) return MM_OK;
    void *p = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
    if (e != hipSuccess) {
        g_last_error = std::string("hipHostMalloc: ") + hipGetErrorString(e);
        return MM_ERR_ALLOC;
    }
    *out = p;
    return MM_OK;
}

void mm_host_free(void *p) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (p) hipHostFree(p);
}

// Host entry point for SHORT sequences (round 5; VERDICT r4: "one short sequence per call costs 28 us whatever its length" -
// and 58-70 us from host memory: an upload, the launch, a download, two waits).  Up to kSmallBases bases the call makes no
// copy through the runtime at all: the bytes are copied by the CPU into a page-locked staging area the device addresses
// (hipHostMallocMapped), the kernel reads them from there and stores its positions (and indices) there, the one wait of the
// synchronous run covers everything, and the CPU copies the results out.  A 150-base read moves 38 bytes in and about 100
// out over the link; what the call costs is the launch and the wait.  (Many reads per call: mm_run_packed_reads_host.)
static const int MM_SMALL_NOT_TAKEN = 1;  // (run_host_small's answer to a call that is not its to serve; errors are negative)
static const uint64_t kSmallBases = 64ull << 10;
static const uint64_t kSmallInBytes = (kSmallBases + 3) / 4 + 64;                 // bytes in, with room for a base offset
static const uint64_t kSmallOutElems = kSmallBases;                               // at most one position per window
static int run_host_small(const mm_plan_t *plan, mm_workspace_t *ws, const HostCall &c) {
    const uint8_t *const packed = static_cast<const uint8_t *>(c.packed);
    const uint64_t base_offset = c.base_offset, n_bases = c.n_bases, capacity = c.capacity;
    uint32_t *const out_pos = c.out_pos, *const out_sk = c.out_sk;
    uint64_t *const out_count = c.out_count;
    const uint64_t bytes = (base_offset + n_bases + 3) / 4;
    if (!ws->h_total_dev || n_bases > kSmallBases || bytes + 16 > kSmallInBytes || mm::mm_env("MM_NO_SMALL_HOST")) return MM_SMALL_NOT_TAKEN;
    const uint64_t in_room = (kSmallInBytes + 255) & ~255ull;
    if (!ws->h_small) {
        void *hp = nullptr, *dp = nullptr;
        // (coherent: the CPU rewrites the bytes between calls and reads the positions right behind the wait - the device must
        // not keep either in its L2, whatever HIP_HOST_COHERENT says)
        if (hipHostMalloc(&hp, in_room + 2 * kSmallOutElems * sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
            hipHostGetDevicePointer(&dp, hp, 0) != hipSuccess) {
            (void)hipGetLastError();
            if (hp) hipHostFree(hp);
            return MM_SMALL_NOT_TAKEN;  // (no mapped host memory on this runtime: the copies below stay)
        }
        ws->h_small = static_cast<uint8_t *>(hp);
        ws->h_small_dev = static_cast<uint8_t *>(dp);
    }
    const uint64_t l = (uint64_t)plan->k + plan->w - 1;
    const uint64_t n_w = n_bases >= l ? n_bases - l + 1 : 0;
    const uint64_t cap = out_pos ? (capacity < n_w ? capacity : n_w) : 0;
    if (bytes) memcpy(ws->h_small, packed, bytes);
    memset(ws->h_small + bytes, 0, 16);
    uint32_t *h_pos = reinterpret_cast<uint32_t *>(ws->h_small + in_room), *h_sk = h_pos + kSmallOutElems;
    uint32_t *d_pos = reinterpret_cast<uint32_t *>(ws->h_small_dev + in_room), *d_sk = d_pos + kSmallOutElems;
    uint64_t count = 0;
    const int r = run_device_sync(plan, ws, {.d_packed = ws->h_small_dev, .packed_bytes = bytes + 16, .base_offset = base_offset,
                                             .n_bases = n_bases, .win_end = UINT64_MAX, .d_out_pos = cap ? d_pos : nullptr,
                                             .d_out_sk = (out_sk && cap) ? d_sk : nullptr, .capacity = cap}, &count);
    if (out_count) *out_count = count;
    if (r) return r;
    if (out_pos && count) {
        memcpy(out_pos, h_pos, count * sizeof(uint32_t));
        if (out_sk) memcpy(out_sk, h_sk, count * sizeof(uint32_t));
    }
    return MM_OK;
}

int mm_run_host(const mm_plan_t *plan, mm_workspace_t *ws, const uint8_t *packed,
                uint64_t base_offset, uint64_t n_bases, uint32_t *out_pos, uint32_t *out_sk,
                uint64_t capacity, uint64_t *out_count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (const int bad = dna_plan_only(plan)) return bad;
    if (!plan || !ws) return MM_ERR_NULL;
    if (n_bases >= (1ull << 32)) return MM_ERR_LEN_TOO_LARGE;
    if (out_sk && plan->mode != MM_MINIMIZERS) return MM_ERR_BAD_MODE;
    MM_HIP(set_device(ws->device));
    const uint64_t bytes = (base_offset + n_bases + 3) / 4;
    if (bytes && !packed) return MM_ERR_NULL;
    HostCall c{.packed = packed, .packed_bytes = bytes, .base_offset = base_offset, .n_bases = n_bases, .out_pos = out_pos,
               .out_sk = out_sk, .capacity = capacity, .out_count = out_count};
    {
        const int rs = run_host_small(plan, ws, c);
        if (rs != MM_SMALL_NOT_TAKEN) return rs;
    }
    int r = grow_bytes(ws->d_in, ws->d_in_bytes, bytes + 16);
    if (r) return r;
    if (bytes) {
        if (!packed) return MM_ERR_NULL;
        r = run_host_pipelined(plan, ws, c);
        if (r != MM_PIPE_FALLBACK) return r;
        MM_HIP(hipMemcpyAsync(ws->d_in, packed, bytes, hipMemcpyHostToDevice, ws->stream));
    }
    c.packed = ws->d_in;  // (staged, with the slack the kernels may touch)
    c.packed_bytes = bytes + 16;
    return run_host_common(plan, ws, c, nullptr);
}

// The staging of both packed-reads host entry points, behind their own argument checks: [packed bytes + slack | starts] in
// d_in, the ambiguity bits (amb != null: PackedNSeq reads) in d_amb, positions (and indices) in d_out / d_sk, offsets in d_vals.
struct PackedReadsHostCall {
    const uint8_t *packed, *amb;
    uint64_t n_reads;
    const uint64_t *read_starts;
    uint32_t max_read_len;
    uint32_t *out_pos, *out_sk;
    uint64_t capacity;
    uint64_t *out_offsets, *out_count;
};
static int packed_reads_host_impl(const mm_plan_t *plan, mm_workspace_t *ws, const PackedReadsHostCall &c) {
    const uint8_t *const packed = c.packed, *const amb = c.amb;
    const uint64_t n_reads = c.n_reads;
    const uint64_t *const read_starts = c.read_starts;
    uint32_t *const out_pos = c.out_pos, *const out_sk = c.out_sk;
    uint64_t *const out_count = c.out_count;
    if (out_count) *out_count = 0;
    MM_HIP(set_device(ws->device));
    const uint64_t total_bases = n_reads ? read_starts[n_reads] : 0;
    for (uint64_t r = 0; r < n_reads; ++r)
        if (read_starts[r] > read_starts[r + 1]) return MM_ERR_CAPACITY;  // (starts must not decrease)
    if (total_bases >= (1ull << 32)) return MM_ERR_LEN_TOO_LARGE;
    const uint64_t bytes = (total_bases + 3) / 4, abytes = (total_bases + 7) / 8;
    const uint64_t starts_at = (bytes + 64 + 15) & ~15ull;
    int r = grow_bytes(ws->d_in, ws->d_in_bytes, starts_at + (n_reads + 1) * sizeof(uint64_t));
    if (r == MM_OK && amb) r = grow_bytes(ws->d_amb, ws->d_amb_bytes, abytes + 16);
    if (r) return r;
    const uint64_t cap = capped(out_pos, c.capacity, total_bases);
    r = stage_outputs(ws, cap, out_sk != nullptr);
    if (r == MM_OK) r = grow(ws->d_vals, ws->d_vals_elems, n_reads + 1, sizeof(unsigned long long));
    if (r) return r;
    uint8_t *const din = static_cast<uint8_t *>(ws->d_in), *const damb = static_cast<uint8_t *>(ws->d_amb);
    if (bytes) MM_HIP(hipMemcpyAsync(din, packed, bytes, hipMemcpyHostToDevice, ws->stream));
    MM_HIP(hipMemsetAsync(din + bytes, 0, starts_at - bytes, ws->stream));
    if (amb) {
        if (abytes) MM_HIP(hipMemcpyAsync(damb, amb, abytes, hipMemcpyHostToDevice, ws->stream));
        MM_HIP(hipMemsetAsync(damb + abytes, 0, 16, ws->stream));
    }
    if (n_reads) MM_HIP(hipMemcpyAsync(din + starts_at, read_starts, (n_reads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, ws->stream));
    const AmbArgs a{damb, abytes + 16, 0};
    uint64_t count = 0;
    r = run_reads_sync(plan, ws, {.d_packed = din, .packed_bytes = starts_at, .n_reads = n_reads, .read_len = c.max_read_len,
                                  .d_read_starts = reinterpret_cast<const uint64_t *>(din + starts_at), .total_bases = total_bases,
                                  .d_out_pos = cap ? ws->d_out : nullptr, .d_out_sk = (out_sk && cap) ? ws->d_sk : nullptr,
                                  .capacity = cap, .d_out_offsets = reinterpret_cast<uint64_t *>(ws->d_vals),
                                  .amb = amb ? &a : nullptr}, &count);
    if (out_count) *out_count = count;
    if (r) return r;
    return download_positions(ws, out_pos, out_sk, count, c.out_offsets, n_reads + 1);
}

// Many short sequences from HOST memory in one call (round 4): what a caller that looped Builder::run over its reads
// (src/lib.rs:378; 2-20 ns per base on the reference's CPU, about 28 us per CALL here) does instead - the reads packed
// back to back, their starts, one upload, ONE launch of the reads-mode kernel, one download.
int mm_run_packed_reads_host(const mm_plan_t *plan, mm_workspace_t *ws, const uint8_t *packed, uint64_t n_reads,
                             const uint64_t *read_starts, uint32_t max_read_len, uint32_t *out_pos, uint32_t *out_sk,
                             uint64_t capacity, uint64_t *out_offsets, uint64_t *out_count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (const int bad = dna_plan_only(plan)) return bad;
    if (!plan || !ws || !out_offsets) return MM_ERR_NULL;
    if (n_reads && (!read_starts || !packed)) return MM_ERR_NULL;
    if (out_sk && plan->mode != MM_MINIMIZERS) return MM_ERR_BAD_MODE;
    return packed_reads_host_impl(plan, ws, {.packed = packed, .n_reads = n_reads, .read_starts = read_starts,
                                             .max_read_len = max_read_len, .out_pos = out_pos, .out_sk = out_sk,
                                             .capacity = capacity, .out_offsets = out_offsets, .out_count = out_count});
}

// The same with ambiguity bits (PackedNSeq reads from host memory).
int mm_run_packed_reads_skip_ambiguous_host(const mm_plan_t *plan, mm_workspace_t *ws, const uint8_t *packed,
                                            const uint8_t *amb, uint64_t n_reads, const uint64_t *read_starts,
                                            uint32_t max_read_len, uint32_t *out_pos, uint64_t capacity,
                                            uint64_t *out_offsets, uint64_t *out_count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    const int c = packed_reads_skip_check(plan, amb, n_reads, read_starts);
    if (c) return c;
    if (!plan || !ws || !out_offsets || (n_reads && !packed)) return MM_ERR_NULL;
    // (no reads: the bits are not looked at, like the device entry point's - but the launch still takes the skip path)
    static const uint8_t no_bits = 0;
    return packed_reads_host_impl(plan, ws, {.packed = packed, .amb = amb ? amb : &no_bits, .n_reads = n_reads,
                                             .read_starts = read_starts, .max_read_len = max_read_len, .out_pos = out_pos,
                                             .capacity = capacity, .out_offsets = out_offsets, .out_count = out_count});
}

// The staging of the sequence host entry points other than mm_run_host, behind their own argument checks: `src` is packed
// bytes or (ascii) one byte per base, packed on the device; `skip` runs the skip-ambiguous windows over the bits of `amb`
// (packed source) or over the bits the ASCII packer writes.
// (c.packed: the HOST source; skip != null runs the skip-ambiguous windows, over skip->amb for a packed source)
struct HostAmb {
    const uint8_t *amb;
    uint64_t amb_offset;
};
static int run_host_staged(const mm_plan_t *plan, mm_workspace_t *ws, const HostCall &c, bool ascii, const HostAmb *skip) {
    const uint8_t *const src = static_cast<const uint8_t *>(c.packed), *const amb = skip ? skip->amb : nullptr;
    const uint64_t base_offset = c.base_offset, n_bases = c.n_bases, amb_offset = skip ? skip->amb_offset : 0;
    MM_HIP(set_device(ws->device));
    const uint64_t bytes = (base_offset + n_bases + 3) / 4, abytes = (amb_offset + n_bases + 7) / 8;
    int r = grow_bytes(ws->d_in, ws->d_in_bytes, bytes + 16);
    if (r == MM_OK && skip) r = grow_bytes(ws->d_amb, ws->d_amb_bytes, abytes + 16);
    if (r == MM_OK && ascii) r = grow_bytes(ws->d_ascii, ws->d_ascii_bytes, n_bases + 16);
    if (r) return r;
    uint8_t *const din = static_cast<uint8_t *>(ws->d_in), *const damb = static_cast<uint8_t *>(ws->d_amb);
    if (n_bases) {
        if (!src || (skip && !ascii && !amb)) return MM_ERR_NULL;
        if (ascii) {
            const uint8_t *const dasc = static_cast<const uint8_t *>(ws->d_ascii);
            MM_HIP(hipMemcpyAsync(ws->d_ascii, src, n_bases, hipMemcpyHostToDevice, ws->stream));
            if (skip ? mm::launch_pack_ascii_n(dasc, n_bases, din, damb, ws->stream) : mm::launch_pack_ascii(dasc, n_bases, din, ws->stream))
                return hip_fail(hipGetLastError(), skip ? "pack_ascii_n" : "pack_ascii");
        } else {
            MM_HIP(hipMemcpyAsync(ws->d_in, src, bytes, hipMemcpyHostToDevice, ws->stream));
            if (skip) MM_HIP(hipMemcpyAsync(ws->d_amb, amb, abytes, hipMemcpyHostToDevice, ws->stream));
        }
    }
    const AmbArgs a{ws->d_amb, abytes + 16, amb_offset};
    HostCall staged = c;
    staged.packed = ws->d_in;
    staged.packed_bytes = bytes + 16;
    return run_host_common(plan, ws, staged, skip ? &a : nullptr);
}

int mm_run_host_ascii(const mm_plan_t *plan, mm_workspace_t *ws, const uint8_t *ascii,
                      uint64_t n_bases, uint32_t *out_pos, uint32_t *out_sk, uint64_t capacity,
                      uint64_t *out_count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (const int bad = dna_plan_only(plan)) return bad;
    if (!plan || !ws) return MM_ERR_NULL;
    if (n_bases >= (1ull << 32)) return MM_ERR_LEN_TOO_LARGE;
    if (out_sk && plan->mode != MM_MINIMIZERS) return MM_ERR_BAD_MODE;
    return run_host_staged(plan, ws, {.packed = ascii, .n_bases = n_bases, .out_pos = out_pos, .out_sk = out_sk,
                                      .capacity = capacity, .out_count = out_count}, true, nullptr);
}

// ------------------------------------------------------------------- text
// General byte text (&[u8]): the generic family's text kernels (mm_generic.hip).  The contracts of the packed twins.
// The device copy of a text plan's tables on this workspace: a slot that holds them already, else the next slot of the ring,
// uploaded on the workspace stream (ordered behind every earlier launch that reads the slot's old tables).
static int text_tables_on_device(mm_workspace_t *ws, const mm::TextTables &tt, const mm::TextTables **out) {
    const int S = mm_workspace::kTextTableSlots;
    if (!ws->d_text_tables) {
        MM_HIP(hipMalloc(&ws->d_text_tables, S * sizeof(mm::TextTables)));
        MM_HIP(hipHostMalloc(&ws->h_text_tables, S * sizeof(mm::TextTables), hipHostMallocDefault));
        for (int i = 0; i < S; ++i) MM_HIP(hipEventCreateWithFlags(&ws->ev_text_tables[i], hipEventDisableTiming));
    }
    for (int i = 0; i < S; ++i)
        if (ws->text_slot_used[i] && memcmp(&ws->h_text_tables[i], &tt, sizeof(tt)) == 0) {
            *out = ws->d_text_tables + i;
            return MM_OK;
        }
    const int i = ws->text_slot_next;
    ws->text_slot_next = (i + 1) % S;
    // (the page-locked slot is rewritten only after its previous upload has left it)
    if (ws->text_slot_used[i]) MM_HIP(hipEventSynchronize(ws->ev_text_tables[i]));
    ws->h_text_tables[i] = tt;
    ws->text_slot_used[i] = true;
    MM_HIP(hipMemcpyAsync(ws->d_text_tables + i, ws->h_text_tables + i, sizeof(tt), hipMemcpyHostToDevice, ws->stream));
    MM_HIP(hipEventRecord(ws->ev_text_tables[i], ws->stream));
    *out = ws->d_text_tables + i;
    return MM_OK;
}

// What every text launch takes from its plan: the sizes, the hasher's scalars, its tables on the device.
static int set_text_plan(mm::TextRunArgs &a, const mm_plan_t *plan, mm_workspace_t *ws) {
    set_plan(a, plan);
    a.hash_rc = plan->tt.canonical != 0;
    a.fw0 = plan->tt.fw0;
    a.rc0 = plan->tt.rc0;
    a.rot = plan->tt.rot;
    return text_tables_on_device(ws, plan->tt, &a.tables);
}

static int run_text_async_impl(const mm_plan_t *plan, mm_workspace_t *ws, const TextCall &c) {
    uint64_t win_end = c.win_end, capacity = c.capacity;
    if (!plan || !ws) return MM_ERR_NULL;
    if (!plan->text) return MM_ERR_BAD_MODE;  // (a plan of mm_plan_create: packed entry points only)
    if (c.n >= (1ull << 32)) return MM_ERR_LEN_TOO_LARGE;
    if (c.d_out_sk && plan->mode != MM_MINIMIZERS) return MM_ERR_BAD_MODE;  // src/lib.rs:339
    if (!c.d_out_pos) capacity = 0;
    const uint64_t l = (uint64_t)plan->k + plan->w - 1;
    const uint64_t n_w = c.n >= l ? c.n - l + 1 : 0;
    if (win_end > n_w) win_end = n_w;
    if (c.win_begin < win_end) {  // (every check before the first stream operation)
        if (!c.d_text) return MM_ERR_NULL;
        if (c.text_bytes < c.n) return MM_ERR_CAPACITY;
    }
    MM_HIP(set_device(ws->device));
    MM_HIP(hipMemsetAsync(ws->total, 0, 2 * sizeof(unsigned long long), ws->stream));
    if (c.win_begin < win_end) {
        mm::TextRunArgs a{};
        int r = set_text_plan(a, plan, ws);
        if (r) return r;
        a.text = static_cast<const uint8_t *>(c.d_text);
        a.n = c.n;
        a.win_begin = c.win_begin;
        a.win_end = win_end;
        a.out = out_params(ws, c.d_out_pos, c.d_out_sk, capacity);
        const uint64_t nwin = win_end - c.win_begin;
        const bool fused = !ws->force_generic && mm::text_walk_supported(plan->k, plan->w);
        if (fused) {
            r = grow_status(ws, mm::text_walk_tiles(nwin) + 1);
            if (r) return r;
        } else {
            a.generic_round_windows = nwin < (1ull << 24) ? nwin : (1ull << 24);
            r = grow_bytes(ws->scratch, ws->scratch_bytes, mm::generic_scratch_bytes(a.generic_round_windows, plan->w));
            if (r) return r;
            a.scratch = ws->scratch;
            r = grow_status(ws, mm::generic_status_words(a.generic_round_windows));
            if (r) return r;
        }
        a.out.status = ws->status;
        ws->status_dirty = true;  // (both text families clear and write untagged words)
        TimedLaunch timed(ws);
        r = timed.arm(a);
        if (r) return r;
        if ((fused ? mm::launch_text_walk(a, ws->stream) : mm::launch_generic_text(a, ws->stream)) != 0) return launch_failed();
        timed.done(fused ? MM_PATH_FUSED : MM_PATH_GENERIC);
    }
    if (c.d_count)
        MM_HIP(hipMemcpyAsync(c.d_count, ws->total, sizeof(unsigned long long), hipMemcpyDeviceToDevice, ws->stream));
    return MM_OK;
}

int mm_run_text_device_async(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_text, uint64_t text_bytes,
                             uint64_t n, uint64_t win_begin, uint64_t win_end, uint32_t *d_out_pos,
                             uint32_t *d_out_sk, uint64_t capacity, uint64_t *d_count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (ws) ws->async_unchecked = true;
    return run_text_async_impl(plan, ws, {.d_text = d_text, .text_bytes = text_bytes, .n = n, .win_begin = win_begin,
                                          .win_end = win_end, .d_out_pos = d_out_pos, .d_out_sk = d_out_sk,
                                          .capacity = capacity, .d_count = d_count});
}

static int run_text_sync(const mm_plan_t *plan, mm_workspace_t *ws, const TextCall &c, uint64_t *out_count) {
    return run_sync(ws, c.capacity, c.d_out_pos != nullptr, out_count, [&](bool *) { return run_text_async_impl(plan, ws, c); });
}

int mm_run_text_device(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_text, uint64_t text_bytes,
                       uint64_t n, uint64_t win_begin, uint64_t win_end, uint32_t *d_out_pos, uint32_t *d_out_sk,
                       uint64_t capacity, uint64_t *out_count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    return run_text_sync(plan, ws, {.d_text = d_text, .text_bytes = text_bytes, .n = n, .win_begin = win_begin,
                                    .win_end = win_end, .d_out_pos = d_out_pos, .d_out_sk = d_out_sk, .capacity = capacity},
                         out_count);
}

int mm_run_text_host(const mm_plan_t *plan, mm_workspace_t *ws, const uint8_t *text, uint64_t n,
                     uint32_t *out_pos, uint32_t *out_sk, uint64_t capacity, uint64_t *out_count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!plan || !ws) return MM_ERR_NULL;
    if (!plan->text) return MM_ERR_BAD_MODE;
    if (n >= (1ull << 32)) return MM_ERR_LEN_TOO_LARGE;
    if (out_sk && plan->mode != MM_MINIMIZERS) return MM_ERR_BAD_MODE;
    if (n && !text) return MM_ERR_NULL;
    MM_HIP(set_device(ws->device));
    const uint64_t l = (uint64_t)plan->k + plan->w - 1;
    const uint64_t n_w = n >= l ? n - l + 1 : 0;
    const uint64_t cap = capped(out_pos, capacity, n_w);
    int r = grow_bytes(ws->d_ascii, ws->d_ascii_bytes, n + 16);
    if (r == MM_OK) r = stage_outputs(ws, cap, out_sk != nullptr);
    if (r) return r;
    if (n) MM_HIP(hipMemcpyAsync(ws->d_ascii, text, n, hipMemcpyHostToDevice, ws->stream));
    uint64_t count = 0;
    r = run_text_sync(plan, ws, {.d_text = ws->d_ascii, .text_bytes = n, .n = n, .win_end = UINT64_MAX,
                                 .d_out_pos = cap ? ws->d_out : nullptr, .d_out_sk = (out_sk && cap) ? ws->d_sk : nullptr,
                                 .capacity = cap}, &count);
    if (out_count) *out_count = count;
    if (r) return r;
    return download_positions(ws, out_pos, out_sk, count, nullptr, 0);
}

// ------------------------------------------------------------- text batch
// Many records of byte text in one call (Builder::run per record, src/lib.rs:378): record r = bytes [starts[r],
// starts[r+1]) of the text, its record-local positions at out[offsets[r] .. offsets[r+1]).  The fused text kernel takes the
// whole batch in ONE launch (BATCH instances, mm_text_walk_impl.h); plans it does not take run one generic-family launch
// per record in stream order (slow: the starts come back to the host first), each appending to the same output and total.
// The argument checks of the batch entry points, before anything is touched (no workspace needed).
static int text_batch_check(const mm_plan_t *plan, const TextBatchCall &c) {
    if (!plan) return MM_ERR_NULL;
    if (!plan->text) return MM_ERR_BAD_MODE;  // (a plan of mm_plan_create: packed entry points only)
    if (c.n_chars >= (1ull << 32) || c.n_records >= (1ull << 31)) return MM_ERR_LEN_TOO_LARGE;
    if (c.d_out_sk && plan->mode != MM_MINIMIZERS) return MM_ERR_BAD_MODE;  // src/lib.rs:339
    if (!c.d_out_offsets || (c.n_records && !c.d_starts)) return MM_ERR_NULL;
    if (c.n_chars > c.text_bytes) return MM_ERR_CAPACITY;
    if (c.n_chars && !c.d_text) return MM_ERR_NULL;
    return MM_OK;
}

static int run_text_batch_async_impl(const mm_plan_t *plan, mm_workspace_t *ws, const TextBatchCall &c) {
    int r = text_batch_check(plan, c);
    if (r) return r;
    if (!ws) return MM_ERR_NULL;
    const uint64_t capacity = c.d_out_pos ? c.capacity : 0;
    MM_HIP(set_device(ws->device));
    MM_HIP(hipMemsetAsync(ws->total, 0, 2 * sizeof(unsigned long long), ws->stream));
    const uint64_t l = (uint64_t)plan->k + plan->w - 1;
    if (c.n_records == 0 || c.n_chars < l) {  // (no window anywhere: every record's slice is empty)
        MM_HIP(hipMemsetAsync(c.d_out_offsets, 0, (c.n_records + 1) * sizeof(uint64_t), ws->stream));
    } else {
        mm::TextRunArgs a{};
        r = set_text_plan(a, plan, ws);
        if (r) return r;
        a.text = static_cast<const uint8_t *>(c.d_text);
        a.out = out_params(ws, c.d_out_pos, c.d_out_sk, capacity);
        const bool fused = !ws->force_generic && mm::text_walk_supported(plan->k, plan->w);
        if (fused) {
            const uint64_t tiles = mm::text_batch_tiles(c.n_chars);
            r = grow_status(ws, tiles + 1);
            if (r == MM_OK) r = grow(ws->d_text_tiles, ws->d_text_tiles_elems, 2 * tiles, sizeof(unsigned long long));
            if (r) return r;
            a.out.status = ws->status;
            ws->status_dirty = true;  // (the text kernels clear and write untagged words)
            a.n = c.n_chars;
            a.win_end = c.n_chars - l + 1;
            a.batch = true;
            a.starts = c.d_starts;
            a.n_records = c.n_records;
            a.tile_rec = ws->d_text_tiles;
            a.offsets = reinterpret_cast<unsigned long long *>(c.d_out_offsets);
            TimedLaunch timed(ws);
            r = timed.arm(a);
            if (r) return r;
            if (mm::launch_text_walk(a, ws->stream) != 0) return launch_failed();
            timed.done(MM_PATH_FUSED);
        } else {
            // one generic launch per record: the look-back adds the running total to each launch's first tile, so the
            // launches append; record r's offset is that total just before its launch (a device-to-device copy)
            std::vector<uint64_t> hs(c.n_records + 1);
            MM_HIP(hipMemcpyAsync(hs.data(), c.d_starts, (c.n_records + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost,
                                  ws->stream));
            MM_HIP(hipStreamSynchronize(ws->stream));
            uint64_t longest = 0;  // (records clamped into [0, n_chars], whatever the starts hold)
            for (uint64_t q = 0; q < c.n_records; ++q) {
                const uint64_t b = hs[q] < c.n_chars ? hs[q] : c.n_chars;
                const uint64_t e = hs[q + 1] < b ? b : (hs[q + 1] < c.n_chars ? hs[q + 1] : c.n_chars);
                if (e - b > longest) longest = e - b;
            }
            const uint64_t max_windows = longest >= l ? longest - l + 1 : 0;
            const uint64_t round = max_windows < (1ull << 24) ? max_windows : (1ull << 24);
            if (round) {
                r = grow_bytes(ws->scratch, ws->scratch_bytes, mm::generic_scratch_bytes(round, plan->w));
                if (r == MM_OK) r = grow_status(ws, mm::generic_status_words(round));
                if (r) return r;
            }
            a.out.status = ws->status;
            ws->status_dirty = true;
            for (uint64_t q = 0; q < c.n_records; ++q) {
                MM_HIP(hipMemcpyAsync(c.d_out_offsets + q, ws->total, sizeof(uint64_t), hipMemcpyDeviceToDevice, ws->stream));
                const uint64_t b = hs[q] < c.n_chars ? hs[q] : c.n_chars;
                const uint64_t e = hs[q + 1] < b ? b : (hs[q + 1] < c.n_chars ? hs[q + 1] : c.n_chars);
                if (e - b < l) continue;
                a.text = static_cast<const uint8_t *>(c.d_text) + b;
                a.n = e - b;
                a.win_begin = 0;
                a.win_end = e - b - l + 1;
                a.generic_round_windows = a.win_end < round ? a.win_end : round;
                a.scratch = ws->scratch;
                if (mm::launch_generic_text(a, ws->stream) != 0) return launch_failed();  // (these launches are not timed)
            }
            MM_HIP(hipMemcpyAsync(c.d_out_offsets + c.n_records, ws->total, sizeof(uint64_t), hipMemcpyDeviceToDevice,
                                  ws->stream));
            ws->last_path = MM_PATH_GENERIC;
        }
    }
    if (c.d_count)
        MM_HIP(hipMemcpyAsync(c.d_count, ws->total, sizeof(unsigned long long), hipMemcpyDeviceToDevice, ws->stream));
    return MM_OK;
}

int mm_run_text_batch_device_async(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_text, uint64_t text_bytes,
                                   uint64_t n_records, const uint64_t *d_starts, uint64_t n_chars, uint32_t *d_out_pos,
                                   uint32_t *d_out_sk, uint64_t capacity, uint64_t *d_out_offsets, uint64_t *d_count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (ws) ws->async_unchecked = true;
    return run_text_batch_async_impl(plan, ws, {.d_text = d_text, .text_bytes = text_bytes, .n_records = n_records,
                                                .d_starts = d_starts, .n_chars = n_chars, .d_out_pos = d_out_pos,
                                                .d_out_sk = d_out_sk, .capacity = capacity, .d_out_offsets = d_out_offsets,
                                                .d_count = d_count});
}

static int run_text_batch_sync(const mm_plan_t *plan, mm_workspace_t *ws, const TextBatchCall &c, uint64_t *out_count) {
    const int rc = text_batch_check(plan, c);
    if (rc) return rc;
    return run_sync(ws, c.capacity, c.d_out_pos != nullptr, out_count,
                    [&](bool *) { return run_text_batch_async_impl(plan, ws, c); });
}

int mm_run_text_batch_device(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_text, uint64_t text_bytes,
                             uint64_t n_records, const uint64_t *d_starts, uint64_t n_chars, uint32_t *d_out_pos,
                             uint32_t *d_out_sk, uint64_t capacity, uint64_t *d_out_offsets, uint64_t *out_count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    return run_text_batch_sync(plan, ws, {.d_text = d_text, .text_bytes = text_bytes, .n_records = n_records,
                                          .d_starts = d_starts, .n_chars = n_chars, .d_out_pos = d_out_pos,
                                          .d_out_sk = d_out_sk, .capacity = capacity, .d_out_offsets = d_out_offsets},
                               out_count);
}

// --------------------------------------------- text batch, counts on the device
// The same run with its two counts in DEVICE memory (d_counts, the layout mm_fasta_text_device_async writes: characters,
// records), read when the kernels run: loader and run queue back to back, nothing waits for the host.  The host knows
// upper bounds only and sizes the launch from them; the kernels do the rest (mm_text_counts.h, mm_text_walk_impl.h).  The
// reference has no counterpart (Builder::run is synchronous host code, src/lib.rs:378); the results are those of
// mm_run_text_batch_device_async given the counts as host arguments.
// The argument checks, before anything is touched (no workspace needed), in the order of text_batch_check.
static int text_batch_counts_check(const mm_plan_t *plan, const TextBatchCountsCall &c) {
    if (!plan) return MM_ERR_NULL;
    if (!plan->text) return MM_ERR_BAD_MODE;  // (a plan of mm_plan_create: packed entry points only)
    if (c.max_chars >= (1ull << 32) || c.max_records >= (1ull << 31)) return MM_ERR_LEN_TOO_LARGE;
    if (c.d_out_sk && plan->mode != MM_MINIMIZERS) return MM_ERR_BAD_MODE;  // src/lib.rs:339
    if (!c.d_out_offsets || !c.d_counts || (c.max_records && !c.d_starts)) return MM_ERR_NULL;
    if (c.max_chars > c.text_bytes) return MM_ERR_CAPACITY;
    if (c.max_chars && !c.d_text) return MM_ERR_NULL;
    if (!mm::text_walk_supported(plan->k, plan->w)) {
        // (the generic family runs one launch per record: it needs the starts on the host)
        g_last_error = "mm_run_text_batch_counts_device*: w > 128 or k > 1024 has no fused text kernel; read the counts back "
                       "and call mm_run_text_batch_device";
        return MM_ERR_BAD_MODE;
    }
    return MM_OK;
}

static int run_text_batch_counts_async_impl(const mm_plan_t *plan, mm_workspace_t *ws, const TextBatchCountsCall &c) {
    int r = text_batch_counts_check(plan, c);
    if (r) return r;
    if (!ws) return MM_ERR_NULL;
    if (ws->force_generic) {
        g_last_error = "mm_run_text_batch_counts_device*: the generic family (mm_workspace_force_generic) needs the starts on "
                       "the host; read the counts back and call mm_run_text_batch_device";
        return MM_ERR_BAD_MODE;
    }
    MM_HIP(set_device(ws->device));
    mm::TextRunArgs a{};
    r = set_text_plan(a, plan, ws);
    if (r) return r;
    // (grid, look-back words and the tiles' record ranges for the bound: max_chars == 0 is still one tile, which writes
    // offsets[0] and the count)
    const uint64_t tiles = mm::text_batch_tiles(c.max_chars);
    r = grow_status(ws, tiles + 1);
    if (r == MM_OK) r = grow(ws->d_text_tiles, ws->d_text_tiles_elems, 2 * tiles, sizeof(unsigned long long));
    if (r) return r;
    MM_HIP(hipMemsetAsync(ws->total, 0, 2 * sizeof(unsigned long long), ws->stream));
    a.text = static_cast<const uint8_t *>(c.d_text);
    a.out = out_params(ws, c.d_out_pos, c.d_out_sk, c.d_out_pos ? c.capacity : 0);
    a.out.status = ws->status;
    ws->status_dirty = true;  // (the text kernels clear and write untagged words)
    a.n = c.max_chars;        // (win_end stays 0: it comes from the counts, on the device)
    a.batch = true;
    a.starts = c.d_starts;
    a.n_records = c.max_records;
    a.tile_rec = ws->d_text_tiles;
    a.offsets = reinterpret_cast<unsigned long long *>(c.d_out_offsets);
    a.counts = c.d_counts;
    TimedLaunch timed(ws);
    r = timed.arm(a);
    if (r) return r;
    if (mm::launch_text_walk(a, ws->stream) != 0) return launch_failed();
    timed.done(MM_PATH_FUSED);
    if (c.d_count)
        MM_HIP(hipMemcpyAsync(c.d_count, ws->total, sizeof(unsigned long long), hipMemcpyDeviceToDevice, ws->stream));
    return MM_OK;
}

int mm_run_text_batch_counts_device_async(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_text,
                                          uint64_t text_bytes, uint64_t max_chars, uint64_t max_records,
                                          const uint64_t *d_starts, const uint64_t *d_counts, uint32_t *d_out_pos,
                                          uint32_t *d_out_sk, uint64_t capacity, uint64_t *d_out_offsets,
                                          uint64_t *d_count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (ws) ws->async_unchecked = true;
    return run_text_batch_counts_async_impl(plan, ws, {.d_text = d_text, .text_bytes = text_bytes, .max_chars = max_chars,
                                                       .max_records = max_records, .d_starts = d_starts, .d_counts = d_counts,
                                                       .d_out_pos = d_out_pos, .d_out_sk = d_out_sk, .capacity = capacity,
                                                       .d_out_offsets = d_out_offsets, .d_count = d_count});
}

int mm_run_text_batch_counts_device(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_text, uint64_t text_bytes,
                                    uint64_t max_chars, uint64_t max_records, const uint64_t *d_starts,
                                    const uint64_t *d_counts, uint32_t *d_out_pos, uint32_t *d_out_sk, uint64_t capacity,
                                    uint64_t *d_out_offsets, uint64_t *out) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    const TextBatchCountsCall c{.d_text = d_text, .text_bytes = text_bytes, .max_chars = max_chars, .max_records = max_records,
                                .d_starts = d_starts, .d_counts = d_counts, .d_out_pos = d_out_pos, .d_out_sk = d_out_sk,
                                .capacity = capacity, .d_out_offsets = d_out_offsets};
    const int rc = text_batch_counts_check(plan, c);
    if (rc) return rc;
    if (!ws) return MM_ERR_NULL;
    return run_counts_sync(ws, d_counts, capacity, d_out_pos != nullptr, out,
                           [&]() { return run_text_batch_counts_async_impl(plan, ws, c); });
}

int mm_run_text_batch_host(const mm_plan_t *plan, mm_workspace_t *ws, const uint8_t *text, uint64_t n_records,
                           const uint64_t *starts, uint32_t *out_pos, uint32_t *out_sk, uint64_t capacity,
                           uint64_t *out_offsets, uint64_t *out_count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!plan || !out_offsets) return MM_ERR_NULL;
    if (!plan->text) return MM_ERR_BAD_MODE;
    if (out_sk && plan->mode != MM_MINIMIZERS) return MM_ERR_BAD_MODE;
    if (n_records && !starts) return MM_ERR_NULL;
    if (n_records >= (1ull << 31)) return MM_ERR_LEN_TOO_LARGE;
    if (out_count) *out_count = 0;
    for (uint64_t q = 0; q < n_records; ++q)
        if (starts[q] > starts[q + 1]) return MM_ERR_UNSORTED;
    const uint64_t n_chars = n_records ? starts[n_records] : 0;
    if (n_chars >= (1ull << 32)) return MM_ERR_LEN_TOO_LARGE;
    if (n_chars && !text) return MM_ERR_NULL;
    if (!ws) return MM_ERR_NULL;
    MM_HIP(set_device(ws->device));
    // staging: [text | starts] in d_in, positions (and indices) in d_out / d_sk, offsets in d_vals
    const uint64_t starts_at = (n_chars + 16 + 15) & ~15ull;
    int r = grow_bytes(ws->d_in, ws->d_in_bytes, starts_at + (n_records + 1) * sizeof(uint64_t));
    if (r) return r;
    const uint64_t cap = capped(out_pos, capacity, n_chars);
    r = stage_outputs(ws, cap, out_sk != nullptr);
    if (r == MM_OK) r = grow(ws->d_vals, ws->d_vals_elems, n_records + 1, sizeof(unsigned long long));
    if (r) return r;
    uint8_t *const din = static_cast<uint8_t *>(ws->d_in);
    if (n_chars) MM_HIP(hipMemcpyAsync(din, text, n_chars, hipMemcpyHostToDevice, ws->stream));
    if (n_records)
        MM_HIP(hipMemcpyAsync(din + starts_at, starts, (n_records + 1) * sizeof(uint64_t), hipMemcpyHostToDevice,
                              ws->stream));
    uint64_t count = 0;
    r = mm_run_text_batch_device(plan, ws, din, n_chars, n_records, reinterpret_cast<const uint64_t *>(din + starts_at),
                                 n_chars, cap ? ws->d_out : nullptr, (out_sk && cap) ? ws->d_sk : nullptr, cap,
                                 reinterpret_cast<uint64_t *>(ws->d_vals), &count);
    if (out_count) *out_count = count;
    if (r) return r;
    return download_positions(ws, out_pos, out_sk, count, out_offsets, n_records + 1);
}

int mm_run_skip_ambiguous_host(const mm_plan_t *plan, mm_workspace_t *ws, const uint8_t *packed,
                               uint64_t base_offset, const uint8_t *amb, uint64_t amb_offset,
                               uint64_t n_bases, uint32_t *out_pos, uint64_t capacity,
                               uint64_t *out_count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (const int bad = dna_plan_only(plan)) return bad;
    if (!plan || !ws) return MM_ERR_NULL;
    if (n_bases >= (1ull << 32)) return MM_ERR_LEN_TOO_LARGE;
    if (!plan->canonical_windows) return MM_ERR_HASHER_NOT_CANONICAL;
    const HostAmb skip{amb, amb_offset};
    return run_host_staged(plan, ws, {.packed = packed, .base_offset = base_offset, .n_bases = n_bases, .out_pos = out_pos,
                                      .capacity = capacity, .out_count = out_count}, false, &skip);
}

int mm_run_skip_ambiguous_host_ascii(const mm_plan_t *plan, mm_workspace_t *ws, const uint8_t *ascii,
                                     uint64_t n_bases, uint32_t *out_pos, uint64_t capacity,
                                     uint64_t *out_count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (const int bad = dna_plan_only(plan)) return bad;
    if (!plan || !ws) return MM_ERR_NULL;
    if (n_bases >= (1ull << 32)) return MM_ERR_LEN_TOO_LARGE;
    if (!plan->canonical_windows) return MM_ERR_HASHER_NOT_CANONICAL;
    const HostAmb skip{nullptr, 0};  // (the bits the ASCII packer writes)
    return run_host_staged(plan, ws, {.packed = ascii, .n_bases = n_bases, .out_pos = out_pos, .capacity = capacity,
                                      .out_count = out_count}, true, &skip);
}

int mm_pack_ascii_n_device_async(mm_workspace_t *ws, const uint8_t *d_ascii, uint64_t n_bases,
                                 uint8_t *d_packed, uint8_t *d_amb) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!ws) return MM_ERR_NULL;
    if (n_bases == 0) return MM_OK;
    if (!d_ascii || !d_packed || !d_amb) return MM_ERR_NULL;
    MM_HIP(set_device(ws->device));
    if (mm::launch_pack_ascii_n(d_ascii, n_bases, d_packed, d_amb, ws->stream))
        return hip_fail(hipGetLastError(), "pack_ascii_n");
    return MM_OK;
}

// ---- Output::values_u64 / values_u128 (src/lib.rs:584-629): `words` 64-bit words per value, 1 or 2
static int values_async_impl(mm_workspace_t *ws, const void *d_packed, uint64_t packed_bytes, uint64_t base_offset,
                             uint64_t n_bases, uint32_t len, int canonical, const uint32_t *d_pos, uint64_t n_pos,
                             uint64_t *d_values, int words) {
    if (!ws) return MM_ERR_NULL;
    if (len == 0 || len > 32u * words) return MM_ERR_VALUE_LEN;
    if (n_pos == 0) return MM_OK;
    if (!d_packed || !d_pos || !d_values) return MM_ERR_NULL;
    MM_HIP(set_device(ws->device));
    mm::SeqView v;
    int r = make_view(d_packed, packed_bytes, base_offset, n_bases, &v);
    if (r) return r;
    unsigned long long *const out = reinterpret_cast<unsigned long long *>(d_values);
    if (words == 2 ? mm::launch_values_u128(v, len, canonical, d_pos, n_pos, out, ws->stream)
                   : mm::launch_values_u64(v, len, canonical, d_pos, n_pos, out, ws->stream))
        return hip_fail(hipGetLastError(), words == 2 ? "values_u128" : "values_u64");
    return MM_OK;
}

// ---- host staging of the whole values family (the *_host entry points): what a value is read from in d_in, the
// positions in d_out, the values in d_vals, `per` 64-bit words each.
// Before anything is queued: `in_bytes` of d_in, room for n_pos positions and their values.
static int values_host_grow(mm_workspace_t *ws, uint64_t in_bytes, uint64_t n_pos, uint64_t per) {
    int r = grow_bytes(ws->d_in, ws->d_in_bytes, in_bytes);
    if (r) return r;
    r = grow(ws->d_out, ws->d_out_elems, n_pos, sizeof(uint32_t));
    if (r) return r;
    return grow(ws->d_vals, ws->d_vals_elems, per * n_pos, sizeof(unsigned long long));
}
// Behind the uploads into d_in: the positions.
static int values_host_upload_pos(mm_workspace_t *ws, const uint32_t *pos, uint64_t n_pos) {
    MM_HIP(hipMemcpyAsync(ws->d_out, pos, n_pos * sizeof(uint32_t), hipMemcpyHostToDevice, ws->stream));
    return MM_OK;
}
// Behind the launch: the values, and the call's one wait.
static int values_host_download(mm_workspace_t *ws, uint64_t *values, uint64_t n_pos, uint64_t per) {
    MM_HIP(hipMemcpyAsync(values, ws->d_vals, per * n_pos * sizeof(uint64_t), hipMemcpyDeviceToHost, ws->stream));
    MM_HIP(hipStreamSynchronize(ws->stream));
    return MM_OK;
}
// The batch-shaped calls' d_in: [payload | starts | offsets], the tables of n + 1 words each at a 16-byte boundary, the
// starts optional (null: a fixed-stride layout).  Grows the three buffers (values_host_grow), then uploads all of d_in;
// d_starts is null with `starts`.
struct ValuesHostTables {
    const uint8_t *d_payload;
    const uint64_t *d_starts, *d_offsets;
};
static int values_host_upload_tables(mm_workspace_t *ws, const uint8_t *payload, uint64_t payload_bytes, uint64_t n,
                                     const uint64_t *starts, const uint64_t *offsets, uint64_t n_pos, uint64_t per,
                                     ValuesHostTables *t) {
    const uint64_t table_bytes = (n + 1) * sizeof(uint64_t);
    const uint64_t starts_at = (payload_bytes + 15) & ~15ull, offsets_at = starts_at + (starts ? table_bytes : 0);
    const int r = values_host_grow(ws, offsets_at + table_bytes, n_pos, per);
    if (r) return r;
    uint8_t *const din = static_cast<uint8_t *>(ws->d_in);
    if (payload_bytes) MM_HIP(hipMemcpyAsync(din, payload, payload_bytes, hipMemcpyHostToDevice, ws->stream));
    if (starts) MM_HIP(hipMemcpyAsync(din + starts_at, starts, table_bytes, hipMemcpyHostToDevice, ws->stream));
    MM_HIP(hipMemcpyAsync(din + offsets_at, offsets, table_bytes, hipMemcpyHostToDevice, ws->stream));
    t->d_payload = din;
    t->d_starts = starts ? reinterpret_cast<const uint64_t *>(din + starts_at) : nullptr;
    t->d_offsets = reinterpret_cast<const uint64_t *>(din + offsets_at);
    return MM_OK;
}

// The same from HOST memory: packed bytes (+ slack for the loads behind the last value) in d_in.
static int values_host_impl(mm_workspace_t *ws, const uint8_t *packed, uint64_t base_offset, uint64_t n_bases, uint32_t len,
                            int canonical, const uint32_t *pos, uint64_t n_pos, uint64_t *values, int words) {
    if (!ws) return MM_ERR_NULL;
    if (len == 0 || len > 32u * words) return MM_ERR_VALUE_LEN;
    if (n_pos == 0) return MM_OK;
    if (!packed || !pos || !values) return MM_ERR_NULL;
    MM_HIP(set_device(ws->device));
    const uint64_t bytes = (base_offset + n_bases + 3) / 4, slack = 16 * words;
    int r = values_host_grow(ws, bytes + slack, n_pos, words);
    if (r) return r;
    MM_HIP(hipMemcpyAsync(ws->d_in, packed, bytes, hipMemcpyHostToDevice, ws->stream));
    r = values_host_upload_pos(ws, pos, n_pos);
    if (r) return r;
    r = values_async_impl(ws, ws->d_in, bytes + slack, base_offset, n_bases, len, canonical, ws->d_out, n_pos,
                          reinterpret_cast<uint64_t *>(ws->d_vals), words);
    if (r) return r;
    return values_host_download(ws, values, n_pos, words);
}

int mm_values_u64_device_async(mm_workspace_t *ws, const void *d_packed, uint64_t packed_bytes,
                               uint64_t base_offset, uint64_t n_bases, uint32_t len,
                               int canonical, const uint32_t *d_pos, uint64_t n_pos,
                               uint64_t *d_values) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    return values_async_impl(ws, d_packed, packed_bytes, base_offset, n_bases, len, canonical, d_pos, n_pos, d_values, 1);
}

int mm_values_u64_host(mm_workspace_t *ws, const uint8_t *packed, uint64_t base_offset,
                       uint64_t n_bases, uint32_t len, int canonical, const uint32_t *pos,
                       uint64_t n_pos, uint64_t *values) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    return values_host_impl(ws, packed, base_offset, n_bases, len, canonical, pos, n_pos, values, 1);
}

int mm_values_u128_device_async(mm_workspace_t *ws, const void *d_packed, uint64_t packed_bytes,
                                uint64_t base_offset, uint64_t n_bases, uint32_t len,
                                int canonical, const uint32_t *d_pos, uint64_t n_pos,
                                uint64_t *d_values) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    return values_async_impl(ws, d_packed, packed_bytes, base_offset, n_bases, len, canonical, d_pos, n_pos, d_values, 2);
}

int mm_values_u128_host(mm_workspace_t *ws, const uint8_t *packed, uint64_t base_offset,
                        uint64_t n_bases, uint32_t len, int canonical, const uint32_t *pos,
                        uint64_t n_pos, uint64_t *values) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    return values_host_impl(ws, packed, base_offset, n_bases, len, canonical, pos, n_pos, values, 2);
}

// ---- Output::values_u64 / values_u128 (src/lib.rs:584-629) of every read of one packed buffer in ONE launch: what a loop
// over Builder::run (src/lib.rs:378) and Output::values_* per read computes, from the read-local positions and offsets the
// reads entry points write (mm_values_reads.hip).  The true count is d_out_offsets[n_reads], read on the device.
static int values_reads_async_impl(mm_workspace_t *ws, const void *d_packed, uint64_t packed_bytes, uint64_t base_offset,
                                   uint64_t n_reads, const uint64_t *d_read_starts, uint32_t read_stride, uint32_t len,
                                   int canonical, const uint32_t *d_pos, const uint64_t *d_out_offsets, uint64_t n_pos_max,
                                   uint64_t *d_values, bool u128) {
    if (!ws) return MM_ERR_NULL;
    if (len == 0 || len > (u128 ? 64u : 32u)) return MM_ERR_VALUE_LEN;
    if (n_reads == 0 || n_pos_max == 0) return MM_OK;
    if (!d_packed || !d_pos || !d_out_offsets || !d_values) return MM_ERR_NULL;
    if (n_reads >= (1ull << 32)) return MM_ERR_LEN_TOO_LARGE;
    if (packed_bytes >= (1ull << 60)) return MM_ERR_LEN_TOO_LARGE;
    // what the host can prove about the layout: the buffer's first base, and a fixed-stride layout's last read, lie
    // inside the buffer (starts in device memory are the kernel's to bound: no load leaves the buffer whatever they hold)
    const uint64_t buffer_bases = 4 * packed_bytes;
    if (base_offset > buffer_bases) return MM_ERR_CAPACITY;
    if (!d_read_starts && (n_reads - 1) * (uint64_t)read_stride > buffer_bases - base_offset) return MM_ERR_CAPACITY;
    MM_HIP(set_device(ws->device));
    mm::ValuesReadsArgs a;
    a.view = mm::packed_view((uint64_t)reinterpret_cast<uintptr_t>(d_packed), packed_bytes, base_offset, 4);
    a.n_reads = n_reads;
    a.read_starts = reinterpret_cast<const unsigned long long *>(d_read_starts);
    a.read_stride = read_stride;
    a.len = len;
    a.canonical = canonical ? 1 : 0;
    a.pos = d_pos;
    a.offsets = reinterpret_cast<const unsigned long long *>(d_out_offsets);
    a.n_pos_max = n_pos_max;
    a.out = reinterpret_cast<unsigned long long *>(d_values);
    const int r = mm::launch_values_reads(a, u128, ws->stream);
    if (r == -3) return MM_ERR_LEN_TOO_LARGE;
    if (r) return hip_fail(hipGetLastError(), u128 ? "values_u128_reads" : "values_u64_reads");
    return MM_OK;
}

int mm_values_u64_reads_device_async(mm_workspace_t *ws, const void *d_packed, uint64_t packed_bytes, uint64_t base_offset,
                                     uint64_t n_reads, const uint64_t *d_read_starts, uint32_t read_stride, uint32_t len,
                                     int canonical, const uint32_t *d_pos, const uint64_t *d_out_offsets,
                                     uint64_t n_pos_max, uint64_t *d_values) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    return values_reads_async_impl(ws, d_packed, packed_bytes, base_offset, n_reads, d_read_starts, read_stride, len,
                                   canonical, d_pos, d_out_offsets, n_pos_max, d_values, false);
}

int mm_values_u128_reads_device_async(mm_workspace_t *ws, const void *d_packed, uint64_t packed_bytes, uint64_t base_offset,
                                      uint64_t n_reads, const uint64_t *d_read_starts, uint32_t read_stride, uint32_t len,
                                      int canonical, const uint32_t *d_pos, const uint64_t *d_out_offsets,
                                      uint64_t n_pos_max, uint64_t *d_values) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    return values_reads_async_impl(ws, d_packed, packed_bytes, base_offset, n_reads, d_read_starts, read_stride, len,
                                   canonical, d_pos, d_out_offsets, n_pos_max, d_values, true);
}

// The same from HOST memory: one upload (packed bytes, starts, positions, offsets), one launch, one download.
static int values_reads_host_impl(mm_workspace_t *ws, const uint8_t *packed, uint64_t packed_bytes, uint64_t base_offset,
                                  uint64_t n_reads, const uint64_t *read_starts, uint32_t read_stride, uint32_t len,
                                  int canonical, const uint32_t *pos, const uint64_t *offsets, uint64_t *values, bool u128) {
    if (!ws) return MM_ERR_NULL;
    if (len == 0 || len > (u128 ? 64u : 32u)) return MM_ERR_VALUE_LEN;
    if (n_reads == 0) return MM_OK;
    if (!offsets) return MM_ERR_NULL;
    if (n_reads >= (1ull << 32)) return MM_ERR_LEN_TOO_LARGE;
    for (uint64_t r = 0; r < n_reads; ++r) {
        if (read_starts && read_starts[r] > read_starts[r + 1]) return MM_ERR_UNSORTED;
        if (offsets[r] > offsets[r + 1]) return MM_ERR_UNSORTED;
    }
    const uint64_t n_pos = offsets[n_reads];
    if (n_pos == 0) return MM_OK;
    if (!packed || !pos || !values) return MM_ERR_NULL;
    if (packed_bytes >= (1ull << 60)) return MM_ERR_LEN_TOO_LARGE;
    if (base_offset > 4 * packed_bytes) return MM_ERR_CAPACITY;
    if (read_starts && read_starts[n_reads] > 4 * packed_bytes - base_offset) return MM_ERR_CAPACITY;
    if (!read_starts && (n_reads - 1) * (uint64_t)read_stride > 4 * packed_bytes - base_offset) return MM_ERR_CAPACITY;
    MM_HIP(set_device(ws->device));
    const uint64_t per = u128 ? 2 : 1;
    ValuesHostTables t;
    int r = values_host_upload_tables(ws, packed, packed_bytes, n_reads, read_starts, offsets, n_pos, per, &t);
    if (r) return r;
    r = values_host_upload_pos(ws, pos, n_pos);
    if (r) return r;
    r = values_reads_async_impl(ws, t.d_payload, packed_bytes, base_offset, n_reads, t.d_starts, read_stride, len, canonical,
                                ws->d_out, t.d_offsets, n_pos, reinterpret_cast<uint64_t *>(ws->d_vals), u128);
    if (r) return r;
    return values_host_download(ws, values, n_pos, per);
}

int mm_values_u64_reads_host(mm_workspace_t *ws, const uint8_t *packed, uint64_t packed_bytes, uint64_t base_offset,
                             uint64_t n_reads, const uint64_t *read_starts, uint32_t read_stride, uint32_t len, int canonical,
                             const uint32_t *pos, const uint64_t *offsets, uint64_t *values) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    return values_reads_host_impl(ws, packed, packed_bytes, base_offset, n_reads, read_starts, read_stride, len, canonical,
                                  pos, offsets, values, false);
}

int mm_values_u128_reads_host(mm_workspace_t *ws, const uint8_t *packed, uint64_t packed_bytes, uint64_t base_offset,
                              uint64_t n_reads, const uint64_t *read_starts, uint32_t read_stride, uint32_t len, int canonical,
                              const uint32_t *pos, const uint64_t *offsets, uint64_t *values) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    return values_reads_host_impl(ws, packed, packed_bytes, base_offset, n_reads, read_starts, read_stride, len, canonical,
                                  pos, offsets, values, true);
}

// The kernel's read lookup on the host (no device): out_read[j] = the read of value idx[j], the largest r in
// [0, n_reads] with offsets[r] <= idx[j] (-1 if there is none) = searchsorted(offsets, idx[j], 'right') - 1.
int mm_debug_values_read_of(const uint64_t *offsets, uint64_t n_reads, const uint64_t *idx, uint64_t n, int64_t *out_read) {
    if (!offsets || (n && (!idx || !out_read))) return MM_ERR_NULL;
    for (uint64_t j = 0; j < n; ++j)
        out_read[j] = idx[j] < offsets[0] ? -1 : (int64_t)mm::values_read_of(offsets, (uint64_t)0, n_reads, idx[j]);
    return MM_OK;
}

uint32_t mm_values_reads_lds_stage(void) { return mm::kValuesReadsStage; }

// ---- one_minimizer(seq, hasher) (src/minimizers.rs:22-28, re-exported at src/lib.rs:211) of EVERY record of a packed
// buffer or of a byte text in one call (mm_one_min.hip): out[r] = the leftmost position that minimises hash & 0xffff0000
// over record r's k-mers, MM_NO_MINIMIZER for a record shorter than k.  No strand vote: the reference has no
// one_canonical_minimizer (FIXME at src/minimizers.rs:30), a canonical hasher only changes the hash.
namespace {

// The rolling tables over the 4 packed symbols: make_text_tables' algebra.
struct OneMinDnaTables {
    mm::OneMinPair t_in[4], t_out[4];
    uint32_t fw0, rc0, rot, canonical;
};
OneMinDnaTables one_min_dna_tables(const mm_hasher_t &h, uint32_t k) {
    OneMinDnaTables t;
    const uint32_t R = h.rot & 31u;
    const uint32_t df = rotl32(h.fw_xor, R) ^ h.fw_xor, dr = rotr32(h.rc_xor, R) ^ h.rc_xor;
    for (int c = 0; c < 4; ++c) {
        t.t_in[c].x = h.fw[c] ^ df;
        t.t_in[c].y = rotl32(h.rc[c], (uint32_t)(((uint64_t)R * (k - 1)) & 31u)) ^ dr;
        t.t_out[c].x = rotl32(h.fw[c], (uint32_t)(((uint64_t)R * k) & 31u));
        t.t_out[c].y = rotr32(h.rc[c], R);
    }
    t.fw0 = h.fw_xor;
    t.rc0 = h.rc_xor;
    t.rot = R;
    t.canonical = h.canonical ? 1u : 0u;
    return t;
}

// The checks that need no device, in the order the header states: MM_ERR_NULL, MM_ERR_K_ZERO, then the layout.  `symbols`:
// what the buffer holds from symbol 0 (packed: 4 * packed_bytes - base_offset, checked here; text: text_bytes).
// host_starts: the starts when the caller has them on the host (host and debug forms), else null.  MM_OK with n == 0:
// nothing to do.  amb (the skip-ambiguous forms, else null): a null buffer is MM_ERR_NULL where a null packed buffer is, an
// amb_offset past its bits MM_ERR_CAPACITY behind the base_offset check.
struct OneMinAmbBits {
    const void *bits;
    uint64_t bytes, offset;
    uint64_t held() const { return bytes >= (1ull << 61) ? ~0ull : 8 * bytes; }  // (bits; saturated, never wraps)
};
int one_min_check(const void *hasher, uint32_t k, const void *data, uint64_t data_bytes, bool packed, uint64_t base_offset,
                  uint64_t n, bool have_starts, const uint64_t *host_starts, uint32_t stride, uint32_t len, const void *out,
                  const OneMinAmbBits *amb = nullptr) {
    if (!hasher) return MM_ERR_NULL;
    if (n && (!out || (!data && data_bytes) || (amb && !amb->bits))) return MM_ERR_NULL;
    if (k == 0) return MM_ERR_K_ZERO;
    if (n == 0) return MM_OK;
    if (n >= (1ull << 32) || data_bytes >= (1ull << 60)) return MM_ERR_LEN_TOO_LARGE;
    const uint64_t buffer = packed ? 4 * data_bytes : data_bytes;
    if (base_offset > buffer) return MM_ERR_CAPACITY;
    if (amb && amb->offset > amb->held()) return MM_ERR_CAPACITY;
    const uint64_t symbols = buffer - base_offset;
    if (!have_starts) {
        if (len > stride) return MM_ERR_BAD_MODE;
        if ((n - 1) * (uint64_t)stride + len > symbols) return MM_ERR_CAPACITY;
    } else if (host_starts) {
        for (uint64_t r = 0; r < n; ++r) {
            if (host_starts[r] > host_starts[r + 1]) return MM_ERR_UNSORTED;
            if (host_starts[r + 1] - host_starts[r] >= 0xFFFFFFFFull) return MM_ERR_LEN_TOO_LARGE;
        }
        if (host_starts[n] > symbols) return MM_ERR_CAPACITY;
    }
    return MM_OK;
}

int one_min_keys(mm_workspace_t *ws, uint64_t n) {
    return grow(ws->d_one_min_keys, ws->d_one_min_keys_elems, n, sizeof(unsigned long long));
}

int one_min_launch(mm_workspace_t *ws, const mm::OneMinArgs &a, const char *what) {
    const int r = mm::launch_one_min(a, ws->stream);
    if (r == -3) return MM_ERR_LEN_TOO_LARGE;
    if (r) return hip_fail(hipGetLastError(), what);
    return MM_OK;
}

// The launch arguments of the packed forms: `avail` symbols behind base_offset (host-n: what the buffer holds; counts: the
// bound max_bases), n records (or their bound).  amb (device bits, or null): a k-mer beyond EITHER buffer does not exist,
// so avail is cut to the bits the ambiguity buffer holds behind amb_offset - the kernels then load no byte outside it.
void one_min_dna_args(mm::OneMinArgs &a, mm_workspace_t *ws, const mm_hasher_t &hasher, uint32_t k, const void *d_packed,
                      uint64_t base_offset, uint64_t avail, uint64_t n, const uint64_t *d_read_starts, uint32_t *d_out_pos,
                      const OneMinAmbBits *amb) {
    const OneMinDnaTables t = one_min_dna_tables(hasher, k);
    a = {};
    a.syms = static_cast<const uint8_t *>(d_packed);
    a.base0 = base_offset;
    a.avail = avail;
    a.n = n;
    a.starts = reinterpret_cast<const unsigned long long *>(d_read_starts);
    a.k = k;
    a.text = false;
    for (int c = 0; c < 4; ++c) {
        a.small_in[c] = make_uint2(t.t_in[c].x, t.t_in[c].y);
        a.small_out[c] = make_uint2(t.t_out[c].x, t.t_out[c].y);
    }
    a.tables = nullptr;
    a.fw0 = t.fw0, a.rc0 = t.rc0, a.rot = t.rot, a.canonical = t.canonical;
    a.keys = ws->d_one_min_keys;
    a.out = d_out_pos;
    if (amb) {
        a.amb = static_cast<const uint8_t *>(amb->bits);
        a.amb0 = amb->offset;
        const uint64_t bits = amb->held() - amb->offset;  // (offset <= held(): checked)
        if (bits < a.avail) a.avail = bits;
    }
}

// (after the checks, the workspace's device current)
int one_min_reads_queue(mm_workspace_t *ws, const mm_hasher_t *hasher, uint32_t k, const void *d_packed, uint64_t packed_bytes,
                        uint64_t base_offset, uint64_t n_reads, const uint64_t *d_read_starts, uint32_t read_stride,
                        uint32_t read_len, uint32_t *d_out_pos, const OneMinAmbBits *amb = nullptr) {
    const int r = one_min_keys(ws, n_reads);
    if (r) return r;
    mm::OneMinArgs a;
    one_min_dna_args(a, ws, *hasher, k, d_packed, base_offset, 4 * packed_bytes - base_offset, n_reads, d_read_starts, d_out_pos,
                     amb);
    a.stride = read_stride;
    a.len = read_len;
    return one_min_launch(ws, a, amb ? "one_minimizer_reads_skip_ambiguous" : "one_minimizer_reads");
}

int one_min_text_queue(mm_workspace_t *ws, const mm_text_hasher_t *hasher, uint32_t k, const void *d_text, uint64_t text_bytes,
                       uint64_t n_records, const uint64_t *d_starts, uint32_t *d_out_pos) {
    int r = one_min_keys(ws, n_records);
    if (r) return r;
    const mm::TextTables tt = make_text_tables(*hasher, k);
    mm::OneMinArgs a = {};
    r = text_tables_on_device(ws, tt, &a.tables);
    if (r) return r;
    a.syms = static_cast<const uint8_t *>(d_text);
    a.base0 = 0;
    a.avail = text_bytes;
    a.n = n_records;
    a.starts = reinterpret_cast<const unsigned long long *>(d_starts);
    a.k = k;
    a.text = true;
    a.fw0 = tt.fw0, a.rc0 = tt.rc0, a.rot = tt.rot, a.canonical = tt.canonical;
    a.keys = ws->d_one_min_keys;
    a.out = d_out_pos;
    return one_min_launch(ws, a, "one_minimizer_text_batch");
}

// The counts forms' checks, before anything is touched, in the order of one_min_check: MM_ERR_NULL (d_counts included),
// MM_ERR_K_ZERO, [max_records == 0: MM_OK], MM_ERR_LEN_TOO_LARGE, MM_ERR_CAPACITY.  `symbols`: what the buffer holds
// (text: text_bytes; packed: 4 * packed_bytes, base_offset + max_sym must lie inside).
// amb (the skip-ambiguous form, else null): as in one_min_check, and amb_offset + max_sym must lie inside its bits.
int one_min_counts_check(const mm_workspace_t *ws, const void *hasher, uint32_t k, const void *data, uint64_t symbols,
                         uint64_t base_offset, uint64_t max_sym, uint64_t max_records, const void *d_starts,
                         const void *d_counts, const void *out, const OneMinAmbBits *amb = nullptr) {
    if (!ws || !hasher || !d_counts) return MM_ERR_NULL;
    if (max_records && (!d_starts || !out || (!data && max_sym) || (amb && !amb->bits))) return MM_ERR_NULL;
    if (k == 0) return MM_ERR_K_ZERO;
    if (max_records == 0) return MM_OK;
    if (max_sym >= (1ull << 32) || max_records >= (1ull << 31)) return MM_ERR_LEN_TOO_LARGE;
    if (base_offset > symbols || max_sym > symbols - base_offset) return MM_ERR_CAPACITY;
    if (amb && (amb->offset > amb->held() || max_sym > amb->held() - amb->offset)) return MM_ERR_CAPACITY;
    return MM_OK;
}

// The packed counts forms behind their checks: the hasher of the caller or of a plan (mm_fastx_stream.hip).
int one_min_reads_counts_queue(mm_workspace_t *ws, const mm_hasher_t &hasher, uint32_t k, const void *d_packed,
                               uint64_t base_offset, uint64_t max_bases, uint64_t max_records, const uint64_t *d_read_starts,
                               const uint64_t *d_counts, uint32_t *d_out_pos, const OneMinAmbBits *amb) {
    MM_HIP(set_device(ws->device));
    ws->async_unchecked = true;  // (a refusal is raised in the sticky error word: mm_workspace_check reports it)
    const int r = one_min_keys(ws, max_records);
    if (r) return r;
    mm::OneMinArgs a;
    one_min_dna_args(a, ws, hasher, k, d_packed, base_offset, max_bases, max_records, d_read_starts, d_out_pos, amb);
    a.counts = reinterpret_cast<const unsigned long long *>(d_counts);
    a.error = error_word(ws);
    return one_min_launch(ws, a, amb ? "one_minimizer_reads_skip_ambiguous_counts" : "one_minimizer_reads_counts");
}

// The checks of both packed counts forms, then the queue.
int one_min_reads_counts(mm_workspace_t *ws, const mm_hasher_t *hasher, uint32_t k, const void *d_packed, uint64_t packed_bytes,
                         uint64_t base_offset, uint64_t max_bases, uint64_t max_records, const uint64_t *d_read_starts,
                         const uint64_t *d_counts, uint32_t *d_out_pos, const OneMinAmbBits *amb) {
    const uint64_t buffer = packed_bytes >= (1ull << 62) ? ~0ull : 4 * packed_bytes;  // (bases; saturated, never wraps)
    const int r = one_min_counts_check(ws, hasher, k, d_packed, buffer, base_offset, max_bases, max_records, d_read_starts,
                                       d_counts, d_out_pos, amb);
    if (r || max_records == 0) return r;
    return one_min_reads_counts_queue(ws, *hasher, k, d_packed, base_offset, max_bases, max_records, d_read_starts, d_counts,
                                      d_out_pos, amb);
}

}  // namespace

int mm_one_minimizer_reads_device_async(mm_workspace_t *ws, const mm_hasher_t *hasher, uint32_t k, const void *d_packed,
                                        uint64_t packed_bytes, uint64_t base_offset, uint64_t n_reads,
                                        const uint64_t *d_read_starts, uint32_t read_stride, uint32_t read_len,
                                        uint32_t *d_out_pos) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!ws) return MM_ERR_NULL;
    const int r = one_min_check(hasher, k, d_packed, packed_bytes, true, base_offset, n_reads, d_read_starts != nullptr, nullptr,
                                read_stride, read_len, d_out_pos);
    if (r || n_reads == 0) return r;
    MM_HIP(set_device(ws->device));
    return one_min_reads_queue(ws, hasher, k, d_packed, packed_bytes, base_offset, n_reads, d_read_starts, read_stride, read_len,
                               d_out_pos);
}

// The skip-ambiguous form: out[r] = the leftmost CLEAN position (no ambiguity bit among its k bases) that minimises
// hash & 0xffff0000 over record r's clean positions, MM_NO_MINIMIZER without one.  K-mer-level skipping; the reference has
// no counterpart (one_minimizer takes a plain Seq, src/minimizers.rs:22-28).  Bit numbering:
// mm_run_packed_reads_skip_ambiguous_device_async's.
int mm_one_minimizer_reads_skip_ambiguous_device_async(mm_workspace_t *ws, const mm_hasher_t *hasher, uint32_t k,
                                                       const void *d_packed, uint64_t packed_bytes, uint64_t base_offset,
                                                       const void *d_amb, uint64_t amb_bytes, uint64_t amb_offset, uint64_t n_reads,
                                                       const uint64_t *d_read_starts, uint32_t read_stride, uint32_t read_len,
                                                       uint32_t *d_out_pos) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!ws) return MM_ERR_NULL;
    const OneMinAmbBits amb{d_amb, amb_bytes, amb_offset};
    const int r = one_min_check(hasher, k, d_packed, packed_bytes, true, base_offset, n_reads, d_read_starts != nullptr, nullptr,
                                read_stride, read_len, d_out_pos, &amb);
    if (r || n_reads == 0) return r;
    MM_HIP(set_device(ws->device));
    return one_min_reads_queue(ws, hasher, k, d_packed, packed_bytes, base_offset, n_reads, d_read_starts, read_stride, read_len,
                               d_out_pos, &amb);
}

int mm_one_minimizer_text_batch_device_async(mm_workspace_t *ws, const mm_text_hasher_t *hasher, uint32_t k, const void *d_text,
                                             uint64_t text_bytes, uint64_t n_records, const uint64_t *d_starts,
                                             uint32_t *d_out_pos) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!ws || (n_records && !d_starts)) return MM_ERR_NULL;
    const int r = one_min_check(hasher, k, d_text, text_bytes, false, 0, n_records, true, nullptr, 0, 0, d_out_pos);
    if (r || n_records == 0) return r;
    MM_HIP(set_device(ws->device));
    return one_min_text_queue(ws, hasher, k, d_text, text_bytes, n_records, d_starts, d_out_pos);
}

static int one_min_text_counts_queue(mm_workspace_t *ws, const mm::TextTables &tt, uint32_t k, const void *d_text,
                                     uint64_t max_chars, uint64_t max_records, const uint64_t *d_starts,
                                     const uint64_t *d_counts, uint32_t *d_out_pos);
// The same with the two counts (symbols, records) in DEVICE memory, read when the kernels run (mm_one_min.h,
// one_min_counts_view): the call queues behind a loader with no host wait.  The reference has no counterpart (one_minimizer
// is synchronous host code over one sequence, src/minimizers.rs:22-28); out[0 .. n) is what the host-n call writes.
int mm_one_minimizer_text_batch_counts_device_async(mm_workspace_t *ws, const mm_text_hasher_t *hasher, uint32_t k,
                                                    const void *d_text, uint64_t text_bytes, uint64_t max_chars,
                                                    uint64_t max_records, const uint64_t *d_starts, const uint64_t *d_counts,
                                                    uint32_t *d_out_pos) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    const int r = one_min_counts_check(ws, hasher, k, d_text, text_bytes, 0, max_chars, max_records, d_starts, d_counts, d_out_pos);
    if (r || max_records == 0) return r;
    return one_min_text_counts_queue(ws, make_text_tables(*hasher, k), k, d_text, max_chars, max_records, d_starts, d_counts,
                                     d_out_pos);
}

// (after the checks; the tables of one (text hasher, k))
static int one_min_text_counts_queue(mm_workspace_t *ws, const mm::TextTables &tt, uint32_t k, const void *d_text,
                                     uint64_t max_chars, uint64_t max_records, const uint64_t *d_starts,
                                     const uint64_t *d_counts, uint32_t *d_out_pos) {
    MM_HIP(set_device(ws->device));
    ws->async_unchecked = true;  // (a refusal is raised in the sticky error word: mm_workspace_check reports it)
    int r = one_min_keys(ws, max_records);
    if (r) return r;
    mm::OneMinArgs a = {};
    r = text_tables_on_device(ws, tt, &a.tables);
    if (r) return r;
    a.syms = static_cast<const uint8_t *>(d_text);
    a.avail = max_chars;
    a.n = max_records;
    a.starts = reinterpret_cast<const unsigned long long *>(d_starts);
    a.k = k;
    a.text = true;
    a.fw0 = tt.fw0, a.rc0 = tt.rc0, a.rot = tt.rot, a.canonical = tt.canonical;
    a.keys = ws->d_one_min_keys;
    a.out = d_out_pos;
    a.counts = reinterpret_cast<const unsigned long long *>(d_counts);
    a.error = error_word(ws);
    return one_min_launch(ws, a, "one_minimizer_text_batch_counts");
}

int mm_one_minimizer_reads_counts_device_async(mm_workspace_t *ws, const mm_hasher_t *hasher, uint32_t k, const void *d_packed,
                                               uint64_t packed_bytes, uint64_t base_offset, uint64_t max_bases,
                                               uint64_t max_records, const uint64_t *d_read_starts, const uint64_t *d_counts,
                                               uint32_t *d_out_pos) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    return one_min_reads_counts(ws, hasher, k, d_packed, packed_bytes, base_offset, max_bases, max_records, d_read_starts,
                                d_counts, d_out_pos, nullptr);
}

// The skip-ambiguous counts form: word for word the plain counts form's contract, over clean k-mers only.
int mm_one_minimizer_reads_skip_ambiguous_counts_device_async(mm_workspace_t *ws, const mm_hasher_t *hasher, uint32_t k,
                                                              const void *d_packed, uint64_t packed_bytes, uint64_t base_offset,
                                                              const void *d_amb, uint64_t amb_bytes, uint64_t amb_offset,
                                                              uint64_t max_bases, uint64_t max_records,
                                                              const uint64_t *d_read_starts, const uint64_t *d_counts,
                                                              uint32_t *d_out_pos) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    const OneMinAmbBits amb{d_amb, amb_bytes, amb_offset};
    return one_min_reads_counts(ws, hasher, k, d_packed, packed_bytes, base_offset, max_bases, max_records, d_read_starts,
                                d_counts, d_out_pos, &amb);
}

// The same from HOST memory: one upload (the bytes the records cover, the starts), the launches, one download.
// (amb: host bits for the skip-ambiguous form, uploaded behind the starts; else null)
static int one_min_reads_host(mm_workspace_t *ws, const mm_hasher_t *hasher, uint32_t k, const uint8_t *packed,
                              uint64_t packed_bytes, uint64_t base_offset, uint64_t n_reads, const uint64_t *read_starts,
                              uint32_t read_stride, uint32_t read_len, uint32_t *out_pos, const OneMinAmbBits *amb) {
    if (!ws) return MM_ERR_NULL;
    int r = one_min_check(hasher, k, packed, packed_bytes, true, base_offset, n_reads, read_starts != nullptr, read_starts,
                          read_stride, read_len, out_pos, amb);
    if (r || n_reads == 0) return r;
    if (amb && amb->bytes >= (1ull << 60)) return MM_ERR_LEN_TOO_LARGE;
    MM_HIP(set_device(ws->device));
    // staging: [packed bytes | starts | ambiguity bits] in d_in, positions in d_out
    const uint64_t words = n_reads + 1;
    const uint64_t starts_at = (packed_bytes + 15) & ~15ull;
    const uint64_t amb_at = starts_at + (read_starts ? words * sizeof(uint64_t) : 0) + 16;
    r = grow_bytes(ws->d_in, ws->d_in_bytes, amb_at + (amb ? amb->bytes : 0));
    if (r) return r;
    r = grow(ws->d_out, ws->d_out_elems, n_reads, sizeof(uint32_t));
    if (r) return r;
    uint8_t *const din = static_cast<uint8_t *>(ws->d_in);
    if (packed_bytes) MM_HIP(hipMemcpyAsync(din, packed, packed_bytes, hipMemcpyHostToDevice, ws->stream));
    if (read_starts)
        MM_HIP(hipMemcpyAsync(din + starts_at, read_starts, words * sizeof(uint64_t), hipMemcpyHostToDevice, ws->stream));
    OneMinAmbBits d_amb{din + amb_at, amb ? amb->bytes : 0, amb ? amb->offset : 0};
    if (amb && amb->bytes) MM_HIP(hipMemcpyAsync(din + amb_at, amb->bits, amb->bytes, hipMemcpyHostToDevice, ws->stream));
    r = one_min_reads_queue(ws, hasher, k, din, packed_bytes, base_offset, n_reads,
                            read_starts ? reinterpret_cast<const uint64_t *>(din + starts_at) : nullptr, read_stride, read_len,
                            ws->d_out, amb ? &d_amb : nullptr);
    if (r) return r;
    MM_HIP(hipMemcpyAsync(out_pos, ws->d_out, n_reads * sizeof(uint32_t), hipMemcpyDeviceToHost, ws->stream));
    MM_HIP(hipStreamSynchronize(ws->stream));
    return MM_OK;
}

int mm_one_minimizer_reads_host(mm_workspace_t *ws, const mm_hasher_t *hasher, uint32_t k, const uint8_t *packed,
                                uint64_t packed_bytes, uint64_t base_offset, uint64_t n_reads, const uint64_t *read_starts,
                                uint32_t read_stride, uint32_t read_len, uint32_t *out_pos) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    return one_min_reads_host(ws, hasher, k, packed, packed_bytes, base_offset, n_reads, read_starts, read_stride, read_len,
                              out_pos, nullptr);
}

int mm_one_minimizer_reads_skip_ambiguous_host(mm_workspace_t *ws, const mm_hasher_t *hasher, uint32_t k, const uint8_t *packed,
                                               uint64_t packed_bytes, uint64_t base_offset, const uint8_t *amb, uint64_t amb_bytes,
                                               uint64_t amb_offset, uint64_t n_reads, const uint64_t *read_starts,
                                               uint32_t read_stride, uint32_t read_len, uint32_t *out_pos) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    const OneMinAmbBits bits{amb, amb_bytes, amb_offset};
    return one_min_reads_host(ws, hasher, k, packed, packed_bytes, base_offset, n_reads, read_starts, read_stride, read_len,
                              out_pos, &bits);
}

int mm_one_minimizer_text_batch_host(mm_workspace_t *ws, const mm_text_hasher_t *hasher, uint32_t k, const uint8_t *text,
                                     uint64_t text_bytes, uint64_t n_records, const uint64_t *starts, uint32_t *out_pos) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!ws || (n_records && !starts)) return MM_ERR_NULL;
    int r = one_min_check(hasher, k, text, text_bytes, false, 0, n_records, true, starts, 0, 0, out_pos);
    if (r || n_records == 0) return r;
    MM_HIP(set_device(ws->device));
    const uint64_t words = n_records + 1;
    const uint64_t n_chars = starts[n_records];  // (<= text_bytes: checked)
    const uint64_t starts_at = (n_chars + 15) & ~15ull;
    r = grow_bytes(ws->d_in, ws->d_in_bytes, starts_at + words * sizeof(uint64_t));
    if (r) return r;
    r = grow(ws->d_out, ws->d_out_elems, n_records, sizeof(uint32_t));
    if (r) return r;
    uint8_t *const din = static_cast<uint8_t *>(ws->d_in);
    if (n_chars) MM_HIP(hipMemcpyAsync(din, text, n_chars, hipMemcpyHostToDevice, ws->stream));
    MM_HIP(hipMemcpyAsync(din + starts_at, starts, words * sizeof(uint64_t), hipMemcpyHostToDevice, ws->stream));
    r = one_min_text_queue(ws, hasher, k, din, n_chars, n_records, reinterpret_cast<const uint64_t *>(din + starts_at), ws->d_out);
    if (r) return r;
    MM_HIP(hipMemcpyAsync(out_pos, ws->d_out, n_records * sizeof(uint32_t), hipMemcpyDeviceToHost, ws->stream));
    MM_HIP(hipStreamSynchronize(ws->stream));
    return MM_OK;
}

uint32_t mm_one_minimizer_tile(void) { return mm::kOneMinTile; }

// The kernel's per-tile function on the host (no device), tile after tile, the per-tile keys combined by minimum; `tile`
// overrides the tile size (0: the kernel's).  The refusals are the host forms', by the same function.
extern "C++" {
namespace {
template <class Sym, class Lay>
void one_min_debug_run(const Sym &sym, const Lay &lay, uint64_t n, uint64_t symbols, const mm::OneMinTables &t, uint32_t k,
                       uint32_t tile, uint32_t *out_pos) {
    std::vector<uint64_t> keys(n, mm::kOneMinNoKey);
    mm::one_min_host(sym, lay, n, symbols, t, k, tile, keys.data());
    for (uint64_t r = 0; r < n; ++r) out_pos[r] = mm::one_min_position(keys[r]);
}
}  // namespace
}  // extern "C++"

extern "C++" {
namespace {
// Both packed debug forms (amb: host bits, or null); the symbols are cut to the ambiguity buffer's bits as the device
// forms cut them (one_min_dna_args).
int one_min_debug_reads(const mm_hasher_t *hasher, uint32_t k, const uint8_t *packed, uint64_t packed_bytes, uint64_t base_offset,
                        uint64_t n_reads, const uint64_t *read_starts, uint32_t read_stride, uint32_t read_len, uint32_t tile,
                        uint32_t *out_pos, const OneMinAmbBits *amb) {
    const int r = one_min_check(hasher, k, packed, packed_bytes, true, base_offset, n_reads, read_starts != nullptr, read_starts,
                                read_stride, read_len, out_pos, amb);
    if (r || n_reads == 0) return r;
    if (tile == 0) tile = mm::kOneMinTile;
    const OneMinDnaTables d = one_min_dna_tables(*hasher, k);
    const mm::OneMinTables t = {d.t_in, d.t_out, d.fw0, d.rc0, d.rot, d.canonical};
    const mm::OneMinPacked packed_sym{packed, base_offset};
    uint64_t symbols = 4 * packed_bytes - base_offset;
    if (amb && amb->held() - amb->offset < symbols) symbols = amb->held() - amb->offset;
    const auto run = [&](const auto &sym) {
        if (read_starts) {
            one_min_debug_run(sym, mm::OneMinStarts{read_starts}, n_reads, symbols, t, k, tile, out_pos);
        } else if (read_len < k) {
            for (uint64_t i = 0; i < n_reads; ++i) out_pos[i] = MM_NO_MINIMIZER;
        } else {
            one_min_debug_run(sym, mm::OneMinStride{read_stride, read_len}, n_reads, symbols, t, k, tile, out_pos);
        }
    };
    if (amb) run(mm::OneMinPackedAmb{packed_sym, static_cast<const uint8_t *>(amb->bits), amb->offset});
    else run(packed_sym);
    return MM_OK;
}
}  // namespace
}  // extern "C++"

int mm_debug_one_minimizer_reads(const mm_hasher_t *hasher, uint32_t k, const uint8_t *packed, uint64_t packed_bytes,
                                 uint64_t base_offset, uint64_t n_reads, const uint64_t *read_starts, uint32_t read_stride,
                                 uint32_t read_len, uint32_t tile, uint32_t *out_pos) {
    return one_min_debug_reads(hasher, k, packed, packed_bytes, base_offset, n_reads, read_starts, read_stride, read_len, tile,
                               out_pos, nullptr);
}

int mm_debug_one_minimizer_reads_skip_ambiguous(const mm_hasher_t *hasher, uint32_t k, const uint8_t *packed, uint64_t packed_bytes,
                                                uint64_t base_offset, const uint8_t *amb, uint64_t amb_bytes, uint64_t amb_offset,
                                                uint64_t n_reads, const uint64_t *read_starts, uint32_t read_stride,
                                                uint32_t read_len, uint32_t tile, uint32_t *out_pos) {
    const OneMinAmbBits bits{amb, amb_bytes, amb_offset};
    return one_min_debug_reads(hasher, k, packed, packed_bytes, base_offset, n_reads, read_starts, read_stride, read_len, tile,
                               out_pos, &bits);
}

int mm_debug_one_minimizer_text_batch(const mm_text_hasher_t *hasher, uint32_t k, const uint8_t *text, uint64_t text_bytes,
                                      uint64_t n_records, const uint64_t *starts, uint32_t tile, uint32_t *out_pos) {
    if (n_records && !starts) return MM_ERR_NULL;
    const int r = one_min_check(hasher, k, text, text_bytes, false, 0, n_records, true, starts, 0, 0, out_pos);
    if (r || n_records == 0) return r;
    if (tile == 0) tile = mm::kOneMinTile;
    const mm::TextTables tt = make_text_tables(*hasher, k);
    static_assert(sizeof(mm::OneMinPair) == sizeof(uint2), "OneMinPair has uint2's layout");
    const mm::OneMinTables t = {reinterpret_cast<const mm::OneMinPair *>(tt.t_in),
                                reinterpret_cast<const mm::OneMinPair *>(tt.t_out), tt.fw0, tt.rc0, tt.rot, tt.canonical};
    one_min_debug_run(mm::OneMinText{text, 0}, mm::OneMinStarts{starts}, n_records, text_bytes, t, k, tile, out_pos);
    return MM_OK;
}

// The counts forms on the host (no device): the view, and the per-tile function run with the view's (n, limit).
int mm_debug_one_minimizer_counts_view(uint64_t max_sym, uint64_t max_records, uint64_t n_sym, uint64_t n,
                                       const uint64_t *starts, uint64_t out[3]) {
    if (!out) return MM_ERR_NULL;
    if (!starts && n && n <= max_records && n_sym <= max_sym) return MM_ERR_NULL;  // (a refused view reads no start)
    const mm::OneMinCountsView v = mm::one_min_counts_view(starts, max_sym, max_records, n_sym, n);
    out[0] = v.n, out[1] = v.limit, out[2] = v.refused;
    return MM_OK;
}

extern "C++" {
namespace {
// out_pos[0 .. max_records): the view's records from the tiles, MM_NO_MINIMIZER at and past them.  MM_ERR_CAPACITY for a
// refused view (what mm_workspace_check reports behind the device form), the output filled all the same.
template <class Sym>
int one_min_debug_counts_run(const Sym &sym, const uint64_t *starts, uint64_t max_sym, uint64_t max_records,
                             const uint64_t *counts, const mm::OneMinTables &t, uint32_t k, uint32_t tile, uint32_t *out_pos) {
    const mm::OneMinCountsView v = mm::one_min_counts_view(starts, max_sym, max_records, counts[0], counts[1]);
    std::vector<uint64_t> keys(max_records, mm::kOneMinNoKey);
    if (v.n) mm::one_min_host(sym, mm::OneMinStarts{starts}, v.n, v.limit, t, k, tile, keys.data());
    for (uint64_t r = 0; r < max_records; ++r) out_pos[r] = r < v.n ? mm::one_min_position(keys[r]) : MM_NO_MINIMIZER;
    return v.refused ? MM_ERR_CAPACITY : MM_OK;
}
}  // namespace
}  // extern "C++"

int mm_debug_one_minimizer_text_batch_counts(const mm_text_hasher_t *hasher, uint32_t k, const uint8_t *text,
                                             uint64_t text_bytes, uint64_t max_chars, uint64_t max_records,
                                             const uint64_t *starts, const uint64_t *counts, uint32_t tile, uint32_t *out_pos) {
    if (!hasher || !counts) return MM_ERR_NULL;
    if (max_records && (!starts || !out_pos || (!text && max_chars))) return MM_ERR_NULL;
    if (k == 0) return MM_ERR_K_ZERO;
    if (max_records == 0) return MM_OK;
    if (max_chars >= (1ull << 32) || max_records >= (1ull << 31)) return MM_ERR_LEN_TOO_LARGE;
    if (max_chars > text_bytes) return MM_ERR_CAPACITY;
    if (tile == 0) tile = mm::kOneMinTile;
    const mm::TextTables tt = make_text_tables(*hasher, k);
    const mm::OneMinTables t = {reinterpret_cast<const mm::OneMinPair *>(tt.t_in),
                                reinterpret_cast<const mm::OneMinPair *>(tt.t_out), tt.fw0, tt.rc0, tt.rot, tt.canonical};
    return one_min_debug_counts_run(mm::OneMinText{text, 0}, starts, max_chars, max_records, counts, t, k, tile, out_pos);
}

static int one_min_debug_reads_counts(const mm_hasher_t *hasher, uint32_t k, const uint8_t *packed, uint64_t packed_bytes,
                                      uint64_t base_offset, uint64_t max_bases, uint64_t max_records, const uint64_t *read_starts,
                                      const uint64_t *counts, uint32_t tile, uint32_t *out_pos, const OneMinAmbBits *amb) {
    if (!hasher || !counts) return MM_ERR_NULL;
    if (max_records && (!read_starts || !out_pos || (!packed && max_bases) || (amb && !amb->bits))) return MM_ERR_NULL;
    if (k == 0) return MM_ERR_K_ZERO;
    if (max_records == 0) return MM_OK;
    if (max_bases >= (1ull << 32) || max_records >= (1ull << 31)) return MM_ERR_LEN_TOO_LARGE;
    const uint64_t buffer = packed_bytes >= (1ull << 62) ? ~0ull : 4 * packed_bytes;  // (bases; saturated, never wraps)
    if (base_offset > buffer || max_bases > buffer - base_offset) return MM_ERR_CAPACITY;
    if (amb && (amb->offset > amb->held() || max_bases > amb->held() - amb->offset)) return MM_ERR_CAPACITY;
    if (tile == 0) tile = mm::kOneMinTile;
    const OneMinDnaTables d = one_min_dna_tables(*hasher, k);
    const mm::OneMinTables t = {d.t_in, d.t_out, d.fw0, d.rc0, d.rot, d.canonical};
    const mm::OneMinPacked sym{packed, base_offset};
    if (amb)
        return one_min_debug_counts_run(mm::OneMinPackedAmb{sym, static_cast<const uint8_t *>(amb->bits), amb->offset}, read_starts,
                                        max_bases, max_records, counts, t, k, tile, out_pos);
    return one_min_debug_counts_run(sym, read_starts, max_bases, max_records, counts, t, k, tile, out_pos);
}

int mm_debug_one_minimizer_reads_counts(const mm_hasher_t *hasher, uint32_t k, const uint8_t *packed, uint64_t packed_bytes,
                                        uint64_t base_offset, uint64_t max_bases, uint64_t max_records,
                                        const uint64_t *read_starts, const uint64_t *counts, uint32_t tile, uint32_t *out_pos) {
    return one_min_debug_reads_counts(hasher, k, packed, packed_bytes, base_offset, max_bases, max_records, read_starts, counts,
                                      tile, out_pos, nullptr);
}

int mm_debug_one_minimizer_reads_skip_ambiguous_counts(const mm_hasher_t *hasher, uint32_t k, const uint8_t *packed,
                                                       uint64_t packed_bytes, uint64_t base_offset, const uint8_t *amb,
                                                       uint64_t amb_bytes, uint64_t amb_offset, uint64_t max_bases,
                                                       uint64_t max_records, const uint64_t *read_starts, const uint64_t *counts,
                                                       uint32_t tile, uint32_t *out_pos) {
    const OneMinAmbBits bits{amb, amb_bytes, amb_offset};
    return one_min_debug_reads_counts(hasher, k, packed, packed_bytes, base_offset, max_bases, max_records, read_starts, counts,
                                      tile, out_pos, &bits);
}

// ---- Output::values_u64 / values_u128 (src/lib.rs:584-629) of every sequence of a device batch in ONE launch: what the
// loop over Builder::run per contig (bench/src/bin/paper.rs:410-431) and Output::values_* per sequence computes, from the
// arrays mm_run_batch_device takes and the offsets it returns (mm_values_batch.hip).
// The checks that need no device, in the order the header lists them; *count = offsets[n_seqs].  MM_OK with *count == 0:
// nothing to do.
static int values_batch_check(uint64_t n_seqs, const void *const *d_packed, const uint64_t *packed_bytes,
                              const uint64_t *base_offsets, const uint64_t *n_bases, uint32_t len, const uint32_t *d_pos,
                              const uint64_t *offsets, const uint64_t *d_values, bool u128, uint64_t *count) {
    *count = 0;
    if (len == 0 || len > (u128 ? 64u : 32u)) return MM_ERR_VALUE_LEN;
    if (n_seqs == 0) return MM_OK;
    if (!offsets) return MM_ERR_NULL;
    if (n_seqs >= (1ull << 32)) return MM_ERR_LEN_TOO_LARGE;
    for (uint64_t s = 0; s < n_seqs; ++s)
        if (offsets[s] > offsets[s + 1]) return MM_ERR_UNSORTED;
    const uint64_t total = offsets[n_seqs];  // (offsets[0] is 0, as mm_run_batch_device writes it)
    if (total == 0) return MM_OK;
    if (!d_packed || !packed_bytes || !n_bases || !d_pos || !d_values) return MM_ERR_NULL;
    for (uint64_t s = 0; s < n_seqs; ++s) {
        if (offsets[s] == offsets[s + 1]) continue;  // (a sequence without values is never looked at)
        if (!d_packed[s]) return MM_ERR_NULL;
        const uint64_t off = base_offsets ? base_offsets[s] : 0;
        if (packed_bytes[s] >= (1ull << 60) || off >= (1ull << 62) || n_bases[s] >= (1ull << 62)) return MM_ERR_LEN_TOO_LARGE;
        if ((off + n_bases[s] + 3) / 4 > packed_bytes[s]) return MM_ERR_CAPACITY;
    }
    *count = total;
    return MM_OK;
}

static int values_batch_async_impl(mm_workspace_t *ws, uint64_t n_seqs, const void *const *d_packed,
                                   const uint64_t *packed_bytes, const uint64_t *base_offsets, const uint64_t *n_bases,
                                   uint32_t len, int canonical, const uint32_t *d_pos, const uint64_t *offsets,
                                   uint64_t *d_values, bool u128) {
    if (!ws) return MM_ERR_NULL;
    uint64_t total = 0;
    int r = values_batch_check(n_seqs, d_packed, packed_bytes, base_offsets, n_bases, len, d_pos, offsets, d_values, u128, &total);
    if (r || total == 0) return r;
    uint32_t blocks;
    if (mm::values_grid(total, u128, &blocks)) return MM_ERR_LEN_TOO_LARGE;  // (more workgroups than a grid holds)
    MM_HIP(set_device(ws->device));
    // the tables: [n_seqs + 1 offsets | pad to 16 bytes | n_seqs descriptors], built in a page-locked area that is the
    // workspace's own - the caller's arrays are the caller's again on return - and copied to the device tables on the
    // stream (behind every earlier launch that reads them)
    const uint64_t seqs_at = ((n_seqs + 1) * sizeof(uint64_t) + 15) & ~15ull;
    const uint64_t bytes = seqs_at + n_seqs * sizeof(mm::ValuesBatchSeq);
    const int slot = ws->vbatch_slot_next;
    ws->vbatch_slot_next = (slot + 1) % mm_workspace::kValuesBatchSlots;
    if (!ws->ev_vbatch[slot]) MM_HIP(hipEventCreateWithFlags(&ws->ev_vbatch[slot], hipEventDisableTiming));
    // (the area is rewritten - or replaced by a larger one - only after its previous upload has left it)
    if (ws->vbatch_slot_used[slot]) MM_HIP(hipEventSynchronize(ws->ev_vbatch[slot]));
    ws->vbatch_slot_used[slot] = false;
    if (ws->h_vbatch_bytes[slot] < bytes) {
        if (ws->h_vbatch[slot]) MM_HIP(hipHostFree(ws->h_vbatch[slot]));
        ws->h_vbatch[slot] = nullptr;
        ws->h_vbatch_bytes[slot] = 0;
        const uint64_t want = bytes + bytes / 8 + 4096;
        void *hp = nullptr;
        MM_HIP(hipHostMalloc(&hp, want, hipHostMallocDefault));
        ws->h_vbatch[slot] = static_cast<uint8_t *>(hp);
        ws->h_vbatch_bytes[slot] = want;
    }
    r = grow(ws->d_vbatch, ws->d_vbatch_bytes, bytes, 1);
    if (r) return r;
    uint8_t *const h = ws->h_vbatch[slot];
    uint64_t *const h_offsets = reinterpret_cast<uint64_t *>(h);
    mm::ValuesBatchSeq *const h_seqs = reinterpret_cast<mm::ValuesBatchSeq *>(h + seqs_at);
    memcpy(h_offsets, offsets, (n_seqs + 1) * sizeof(uint64_t));
    for (uint64_t s = 0; s < n_seqs; ++s)
        h_seqs[s] = offsets[s] == offsets[s + 1]
                        ? mm::ValuesBatchSeq{0, 0, 0, 0}
                        : mm::values_batch_seq((uint64_t)reinterpret_cast<uintptr_t>(d_packed[s]), packed_bytes[s],
                                               base_offsets ? base_offsets[s] : 0);
    MM_HIP(hipMemcpyAsync(ws->d_vbatch, h, bytes, hipMemcpyHostToDevice, ws->stream));
    MM_HIP(hipEventRecord(ws->ev_vbatch[slot], ws->stream));
    ws->vbatch_slot_used[slot] = true;
    mm::ValuesBatchArgs a;
    a.n_seqs = n_seqs;
    a.seqs = reinterpret_cast<const mm::ValuesBatchSeq *>(ws->d_vbatch + seqs_at);
    a.offsets = reinterpret_cast<const unsigned long long *>(ws->d_vbatch);
    a.total = total;
    a.len = len;
    a.canonical = canonical ? 1 : 0;
    a.pos = d_pos;
    a.out = reinterpret_cast<unsigned long long *>(d_values);
    r = mm::launch_values_batch(a, u128, ws->stream);
    if (r == -3) return MM_ERR_LEN_TOO_LARGE;
    if (r) return hip_fail(hipGetLastError(), u128 ? "values_u128_batch" : "values_u64_batch");
    return MM_OK;
}

int mm_values_u64_batch_device_async(mm_workspace_t *ws, uint64_t n_seqs, const void *const *d_packed,
                                     const uint64_t *packed_bytes, const uint64_t *base_offsets, const uint64_t *n_bases,
                                     uint32_t len, int canonical, const uint32_t *d_pos, const uint64_t *offsets,
                                     uint64_t *d_values) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    return values_batch_async_impl(ws, n_seqs, d_packed, packed_bytes, base_offsets, n_bases, len, canonical, d_pos, offsets,
                                   d_values, false);
}

int mm_values_u128_batch_device_async(mm_workspace_t *ws, uint64_t n_seqs, const void *const *d_packed,
                                      const uint64_t *packed_bytes, const uint64_t *base_offsets, const uint64_t *n_bases,
                                      uint32_t len, int canonical, const uint32_t *d_pos, const uint64_t *offsets,
                                      uint64_t *d_values) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    return values_batch_async_impl(ws, n_seqs, d_packed, packed_bytes, base_offsets, n_bases, len, canonical, d_pos, offsets,
                                   d_values, true);
}

uint32_t mm_values_batch_lds_stage(void) { return mm::kValuesBatchStage; }

// The view the host derives for one sequence of a batch (no device): out6 = {aligned address, byte_lo, byte_hi, q_lo, q_hi,
// base0}, what the kernel reads out of the sequence's descriptor.
int mm_debug_values_batch_view(uint64_t address, uint64_t packed_bytes, uint64_t base_offset, uint64_t out6[6]) {
    if (!out6) return MM_ERR_NULL;
    const mm::PackedView v = mm::view_of(mm::values_batch_seq(address, packed_bytes, base_offset));
    out6[0] = (uint64_t)reinterpret_cast<uintptr_t>(v.d);
    out6[1] = v.byte_lo;
    out6[2] = v.byte_hi;
    out6[3] = v.q_lo;
    out6[4] = v.q_hi;
    out6[5] = v.base0;
    return MM_OK;
}

// ---- Output::values_u64 / values_u128 (src/lib.rs:584-629) of byte text, at the positions the text entry points write
// (mm_values_text.hip).  `encoding` names the reference Seq the text stands for: `&[u8]` (src/lib.rs:59-60) at 8 bits per
// character, or packed-seq AsciiSeq (src/lib.rs:59, :85-100) at 2.
static int values_text_mode_check(int encoding, uint32_t len, int canonical, bool u128) {
    if (encoding != MM_TEXT_VALUES_BYTES && encoding != MM_TEXT_VALUES_DNA) return MM_ERR_BAD_MODE;
    if (encoding == MM_TEXT_VALUES_BYTES && canonical) return MM_ERR_BAD_MODE;  // (general text has no reverse complement)
    const uint32_t most = (encoding == MM_TEXT_VALUES_DNA ? 32u : 8u) * (u128 ? 2u : 1u);
    if (len == 0 || len > most) return MM_ERR_VALUE_LEN;
    return MM_OK;
}

static int values_text_async_impl(mm_workspace_t *ws, const void *d_text, uint64_t text_bytes, uint64_t n, int encoding,
                                  uint32_t len, int canonical, const uint32_t *d_pos, uint64_t n_pos, uint64_t *d_values,
                                  bool u128) {
    if (!ws) return MM_ERR_NULL;
    if (const int bad = values_text_mode_check(encoding, len, canonical, u128)) return bad;
    if (n_pos == 0) return MM_OK;
    if (!d_text || !d_pos || !d_values) return MM_ERR_NULL;
    if (n >= (1ull << 32)) return MM_ERR_LEN_TOO_LARGE;
    if (n > text_bytes) return MM_ERR_CAPACITY;
    MM_HIP(set_device(ws->device));
    mm::ValuesTextArgs a;
    a.view = mm::text_view((uint64_t)reinterpret_cast<uintptr_t>(d_text), text_bytes);
    a.n_records = 0;
    a.starts = nullptr;
    a.len = len;
    a.canonical = canonical ? 1 : 0;
    a.pos = d_pos;
    a.offsets = nullptr;
    a.n_pos_max = n_pos;
    a.out = reinterpret_cast<unsigned long long *>(d_values);
    const int r = mm::launch_values_text(a, encoding, u128, false, ws->stream);
    if (r == -3) return MM_ERR_LEN_TOO_LARGE;
    if (r) return hip_fail(hipGetLastError(), u128 ? "values_u128_text" : "values_u64_text");
    return MM_OK;
}

// The same from HOST memory: the text in d_in (text_bytes = n: a k-mer past the end reads zeros).
static int values_text_host_impl(mm_workspace_t *ws, const uint8_t *text, uint64_t n, int encoding, uint32_t len,
                                 int canonical, const uint32_t *pos, uint64_t n_pos, uint64_t *values, bool u128) {
    if (!ws) return MM_ERR_NULL;
    if (const int bad = values_text_mode_check(encoding, len, canonical, u128)) return bad;
    if (n_pos == 0) return MM_OK;
    if ((n && !text) || !pos || !values) return MM_ERR_NULL;
    if (n >= (1ull << 32)) return MM_ERR_LEN_TOO_LARGE;
    MM_HIP(set_device(ws->device));
    const uint64_t per = u128 ? 2 : 1;
    int r = values_host_grow(ws, n ? n : 1, n_pos, per);
    if (r) return r;
    if (n) MM_HIP(hipMemcpyAsync(ws->d_in, text, n, hipMemcpyHostToDevice, ws->stream));
    r = values_host_upload_pos(ws, pos, n_pos);
    if (r) return r;
    r = values_text_async_impl(ws, ws->d_in, n, n, encoding, len, canonical, ws->d_out, n_pos,
                               reinterpret_cast<uint64_t *>(ws->d_vals), u128);
    if (r) return r;
    return values_host_download(ws, values, n_pos, per);
}

int mm_values_u64_text_device_async(mm_workspace_t *ws, const void *d_text, uint64_t text_bytes, uint64_t n, int encoding,
                                    uint32_t len, int canonical, const uint32_t *d_pos, uint64_t n_pos, uint64_t *d_values) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    return values_text_async_impl(ws, d_text, text_bytes, n, encoding, len, canonical, d_pos, n_pos, d_values, false);
}

int mm_values_u128_text_device_async(mm_workspace_t *ws, const void *d_text, uint64_t text_bytes, uint64_t n, int encoding,
                                     uint32_t len, int canonical, const uint32_t *d_pos, uint64_t n_pos, uint64_t *d_values) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    return values_text_async_impl(ws, d_text, text_bytes, n, encoding, len, canonical, d_pos, n_pos, d_values, true);
}

int mm_values_u64_text_host(mm_workspace_t *ws, const uint8_t *text, uint64_t n, int encoding, uint32_t len, int canonical,
                            const uint32_t *pos, uint64_t n_pos, uint64_t *values) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    return values_text_host_impl(ws, text, n, encoding, len, canonical, pos, n_pos, values, false);
}

int mm_values_u128_text_host(mm_workspace_t *ws, const uint8_t *text, uint64_t n, int encoding, uint32_t len, int canonical,
                             const uint32_t *pos, uint64_t n_pos, uint64_t *values) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    return values_text_host_impl(ws, text, n, encoding, len, canonical, pos, n_pos, values, true);
}

// Every record of a text batch in ONE launch: what a loop over Builder::run per record (src/lib.rs:378) and
// Output::values_* per record computes, from the record-local positions and offsets mm_run_text_batch_device_async
// writes.  The true count is d_out_offsets[n_records], read on the device.
static int values_text_batch_async_impl(mm_workspace_t *ws, const void *d_text, uint64_t text_bytes, uint64_t n_records,
                                        const uint64_t *d_starts, uint64_t n_chars, int encoding, uint32_t len, int canonical,
                                        const uint32_t *d_pos, const uint64_t *d_out_offsets, uint64_t n_pos_max,
                                        uint64_t *d_values, bool u128) {
    if (!ws) return MM_ERR_NULL;
    if (const int bad = values_text_mode_check(encoding, len, canonical, u128)) return bad;
    if (n_records == 0 || n_pos_max == 0) return MM_OK;
    if (!d_text || !d_starts || !d_pos || !d_out_offsets || !d_values) return MM_ERR_NULL;
    if (n_chars >= (1ull << 32) || n_records >= (1ull << 31)) return MM_ERR_LEN_TOO_LARGE;
    if (n_chars > text_bytes) return MM_ERR_CAPACITY;
    MM_HIP(set_device(ws->device));
    mm::ValuesTextArgs a;
    a.view = mm::text_view((uint64_t)reinterpret_cast<uintptr_t>(d_text), text_bytes);
    a.n_records = n_records;
    a.starts = reinterpret_cast<const unsigned long long *>(d_starts);
    a.len = len;
    a.canonical = canonical ? 1 : 0;
    a.pos = d_pos;
    a.offsets = reinterpret_cast<const unsigned long long *>(d_out_offsets);
    a.n_pos_max = n_pos_max;
    a.out = reinterpret_cast<unsigned long long *>(d_values);
    const int r = mm::launch_values_text(a, encoding, u128, true, ws->stream);
    if (r == -3) return MM_ERR_LEN_TOO_LARGE;
    if (r) return hip_fail(hipGetLastError(), u128 ? "values_u128_text_batch" : "values_u64_text_batch");
    return MM_OK;
}

// The same from HOST memory: one upload ([text | starts | offsets] in d_in, positions in d_out), one launch, one download.
static int values_text_batch_host_impl(mm_workspace_t *ws, const uint8_t *text, uint64_t n_records, const uint64_t *starts,
                                       int encoding, uint32_t len, int canonical, const uint32_t *pos, const uint64_t *offsets,
                                       uint64_t *values, bool u128) {
    if (!ws) return MM_ERR_NULL;
    if (const int bad = values_text_mode_check(encoding, len, canonical, u128)) return bad;
    if (n_records == 0) return MM_OK;
    if (!starts || !offsets) return MM_ERR_NULL;
    if (n_records >= (1ull << 31)) return MM_ERR_LEN_TOO_LARGE;
    for (uint64_t r = 0; r < n_records; ++r)
        if (starts[r] > starts[r + 1] || offsets[r] > offsets[r + 1]) return MM_ERR_UNSORTED;
    const uint64_t n_pos = offsets[n_records], n_chars = starts[n_records];
    if (n_pos == 0) return MM_OK;
    if (!text || !pos || !values) return MM_ERR_NULL;
    if (n_chars >= (1ull << 32)) return MM_ERR_LEN_TOO_LARGE;
    MM_HIP(set_device(ws->device));
    const uint64_t per = u128 ? 2 : 1;
    ValuesHostTables t;
    int r = values_host_upload_tables(ws, text, n_chars, n_records, starts, offsets, n_pos, per, &t);
    if (r) return r;
    r = values_host_upload_pos(ws, pos, n_pos);
    if (r) return r;
    // (text_bytes = n_chars: a k-mer that leaves the last record reads zeros, not the staged starts)
    r = values_text_batch_async_impl(ws, t.d_payload, n_chars, n_records, t.d_starts, n_chars, encoding, len, canonical,
                                     ws->d_out, t.d_offsets, n_pos, reinterpret_cast<uint64_t *>(ws->d_vals), u128);
    if (r) return r;
    return values_host_download(ws, values, n_pos, per);
}

int mm_values_u64_text_batch_device_async(mm_workspace_t *ws, const void *d_text, uint64_t text_bytes, uint64_t n_records,
                                          const uint64_t *d_starts, uint64_t n_chars, int encoding, uint32_t len,
                                          int canonical, const uint32_t *d_pos, const uint64_t *d_out_offsets,
                                          uint64_t n_pos_max, uint64_t *d_values) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    return values_text_batch_async_impl(ws, d_text, text_bytes, n_records, d_starts, n_chars, encoding, len, canonical, d_pos,
                                        d_out_offsets, n_pos_max, d_values, false);
}

int mm_values_u128_text_batch_device_async(mm_workspace_t *ws, const void *d_text, uint64_t text_bytes, uint64_t n_records,
                                           const uint64_t *d_starts, uint64_t n_chars, int encoding, uint32_t len,
                                           int canonical, const uint32_t *d_pos, const uint64_t *d_out_offsets,
                                           uint64_t n_pos_max, uint64_t *d_values) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    return values_text_batch_async_impl(ws, d_text, text_bytes, n_records, d_starts, n_chars, encoding, len, canonical, d_pos,
                                        d_out_offsets, n_pos_max, d_values, true);
}

// The values of a counts run (mm_run_text_batch_counts_device_async): the records' number comes from d_counts[1] on the
// device - for the record search and for the true count d_out_offsets[n_records] - and both counts are held against the
// bounds there: beyond them (the state the run refuses) or with no record, nothing is written.
static int values_text_batch_counts_async_impl(mm_workspace_t *ws, const void *d_text, uint64_t text_bytes, uint64_t max_chars,
                                               uint64_t max_records, const uint64_t *d_starts, const uint64_t *d_counts,
                                               int encoding, uint32_t len, int canonical, const uint32_t *d_pos,
                                               const uint64_t *d_out_offsets, uint64_t n_pos_max, uint64_t *d_values,
                                               bool u128) {
    if (!ws) return MM_ERR_NULL;
    if (const int bad = values_text_mode_check(encoding, len, canonical, u128)) return bad;
    if (max_records == 0 || n_pos_max == 0) return MM_OK;
    if (!d_text || !d_starts || !d_counts || !d_pos || !d_out_offsets || !d_values) return MM_ERR_NULL;
    if (max_chars >= (1ull << 32) || max_records >= (1ull << 31)) return MM_ERR_LEN_TOO_LARGE;
    if (max_chars > text_bytes) return MM_ERR_CAPACITY;
    MM_HIP(set_device(ws->device));
    mm::ValuesTextArgs a;
    a.view = mm::text_view((uint64_t)reinterpret_cast<uintptr_t>(d_text), text_bytes);
    a.n_records = max_records;
    a.starts = reinterpret_cast<const unsigned long long *>(d_starts);
    a.len = len;
    a.canonical = canonical ? 1 : 0;
    a.pos = d_pos;
    a.offsets = reinterpret_cast<const unsigned long long *>(d_out_offsets);
    a.n_pos_max = n_pos_max;
    a.out = reinterpret_cast<unsigned long long *>(d_values);
    a.counts = reinterpret_cast<const unsigned long long *>(d_counts);
    a.max_chars = max_chars;
    const int r = mm::launch_values_text(a, encoding, u128, true, ws->stream);
    if (r == -3) return MM_ERR_LEN_TOO_LARGE;
    if (r) return hip_fail(hipGetLastError(), u128 ? "values_u128_text_batch_counts" : "values_u64_text_batch_counts");
    return MM_OK;
}

int mm_values_u64_text_batch_counts_device_async(mm_workspace_t *ws, const void *d_text, uint64_t text_bytes,
                                                 uint64_t max_chars, uint64_t max_records, const uint64_t *d_starts,
                                                 const uint64_t *d_counts, int encoding, uint32_t len, int canonical,
                                                 const uint32_t *d_pos, const uint64_t *d_out_offsets, uint64_t n_pos_max,
                                                 uint64_t *d_values) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    return values_text_batch_counts_async_impl(ws, d_text, text_bytes, max_chars, max_records, d_starts, d_counts, encoding,
                                               len, canonical, d_pos, d_out_offsets, n_pos_max, d_values, false);
}

int mm_values_u128_text_batch_counts_device_async(mm_workspace_t *ws, const void *d_text, uint64_t text_bytes,
                                                  uint64_t max_chars, uint64_t max_records, const uint64_t *d_starts,
                                                  const uint64_t *d_counts, int encoding, uint32_t len, int canonical,
                                                  const uint32_t *d_pos, const uint64_t *d_out_offsets, uint64_t n_pos_max,
                                                  uint64_t *d_values) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    return values_text_batch_counts_async_impl(ws, d_text, text_bytes, max_chars, max_records, d_starts, d_counts, encoding,
                                               len, canonical, d_pos, d_out_offsets, n_pos_max, d_values, true);
}

// What the counts kernels make of {counts, bounds}, by the function they call (mm_text_counts.h): no device.
int mm_debug_text_counts_view(uint32_t k, uint32_t w, uint64_t max_chars, uint64_t max_records, uint64_t n_chars,
                              uint64_t n_records, uint64_t out[4]) {
    if (!out) return MM_ERR_NULL;
    if (w == 0) return MM_ERR_W_ZERO;
    if (max_chars >= (1ull << 32) || max_records >= (1ull << 31)) return MM_ERR_LEN_TOO_LARGE;  // (the entry points' rule)
    const mm::TextCountsView v = mm::text_counts_view(k + w - 1, max_chars, max_records, n_chars, n_records);
    out[0] = v.tiles;
    out[1] = mm::text_counts_tiles(max_chars);
    out[2] = v.win_end;
    out[3] = v.refused;
    return MM_OK;
}

int mm_values_u64_text_batch_host(mm_workspace_t *ws, const uint8_t *text, uint64_t n_records, const uint64_t *starts,
                                  int encoding, uint32_t len, int canonical, const uint32_t *pos, const uint64_t *offsets,
                                  uint64_t *values) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    return values_text_batch_host_impl(ws, text, n_records, starts, encoding, len, canonical, pos, offsets, values, false);
}

int mm_values_u128_text_batch_host(mm_workspace_t *ws, const uint8_t *text, uint64_t n_records, const uint64_t *starts,
                                   int encoding, uint32_t len, int canonical, const uint32_t *pos, const uint64_t *offsets,
                                   uint64_t *values) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    return values_text_batch_host_impl(ws, text, n_records, starts, encoding, len, canonical, pos, offsets, values, true);
}

uint32_t mm_values_text_lds_stage(void) { return mm::kValuesTextStage; }

// The kernels' arithmetic for one value on the host, of a HOST buffer (no device): out[j] (want_u128: out[2j], out[2j + 1])
// = the value at absolute position abs_pos[j], by the functions the kernels call - the gather from whole dwords and
// edge bytes, the 2-bit compression, the assembly and the canonical step (mm_values_text.h).
int mm_debug_values_text(const uint8_t *text, uint64_t text_bytes, int encoding, uint32_t len, int canonical, int want_u128,
                         const uint64_t *abs_pos, uint64_t n, uint64_t *out) {
    if (const int bad = values_text_mode_check(encoding, len, canonical, want_u128 != 0)) return bad;
    if (n == 0) return MM_OK;
    if ((text_bytes && !text) || !abs_pos || !out) return MM_ERR_NULL;
    const mm::PackedView view = mm::text_view((uint64_t)reinterpret_cast<uintptr_t>(text), text_bytes);
    const uint64_t per = want_u128 ? 2 : 1;
    for (uint64_t j = 0; j < n; ++j)
        mm::values_text_host_one(view, encoding, len, canonical ? 1 : 0, want_u128 != 0, abs_pos[j], out + per * j);
    return MM_OK;
}

int mm_pack_ascii_device_async(mm_workspace_t *ws, const uint8_t *d_ascii, uint64_t n_bases,
                               uint8_t *d_packed) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!ws) return MM_ERR_NULL;
    if (n_bases == 0) return MM_OK;
    if (!d_ascii || !d_packed) return MM_ERR_NULL;
    MM_HIP(set_device(ws->device));
    if (mm::launch_pack_ascii(d_ascii, n_bases, d_packed, ws->stream))
        return hip_fail(hipGetLastError(), "pack_ascii");
    return MM_OK;
}

// Which FASTA packer a call takes.  The product has ONE: the two passes of mask arithmetic (mm_fasta2.hip - no
// look-back, no tables with limits, nothing to fall back from).  The packers of rounds 2-4 (mm_fasta.hip: the one-pass
// kernel over lines, 1, and the three-pass kernels, 2) are cross-checks in the EXPERIMENTS build only since round 5
// (VERDICT r4 item 5): MM_FASTA_KERNEL=lines|three / MM_FASTA_ONEPASS=1|0 are read there and nowhere else.
static int fasta_packer_choice(const mm_workspace_t *ws) {
#ifdef MM_EXPERIMENTS
    const char *k = mm::mm_env("MM_FASTA_KERNEL"), *one = mm::mm_env("MM_FASTA_ONEPASS");
    int c = 0;
    if (k) c = !strcmp(k, "lines") ? 1 : (!strcmp(k, "three") ? 2 : 0);
    else if (one) c = one[0] == '0' ? 2 : 1;
    if (c == 1 && (ws->fasta_three_pass || ws->fasta_three_once)) c = 2;
    return c;
#else
    (void)ws;
    return 0;
#endif
}

// What the *_pack_n entry points ask of their second output, before anything else is looked at (no device needed).
static int amb_out_check(const uint8_t *d_amb, uint64_t amb_capacity_bytes) {
    if (!d_amb || reinterpret_cast<uintptr_t>(d_amb) % 4 != 0) return MM_ERR_NULL;
    if (amb_capacity_bytes == 0 || amb_capacity_bytes % 4 != 0) return MM_ERR_CAPACITY;
    return MM_OK;
}

// What the FASTA and the FASTQ packer do before they differ: the argument checks, the workspace's device, and an empty text's
// answer (no base, no record).  Returns MM_PACK_GO_ON when there is a text to pack, else the call's result.
static const int MM_PACK_GO_ON = 1;
static int pack_prologue(mm_workspace_t *ws, const uint8_t *d_text, uint64_t n_bytes, const uint8_t *d_packed,
                         uint64_t packed_capacity_bytes, uint64_t *d_rec_base, uint64_t *d_counts, uint8_t *d_amb,
                         uint64_t amb_capacity_bytes) {
    if (!ws || !d_counts || !d_rec_base) return MM_ERR_NULL;
    if (n_bytes >= (1ull << 32)) return MM_ERR_LEN_TOO_LARGE;
    if (reinterpret_cast<uintptr_t>(d_packed) % 4 != 0) return MM_ERR_NULL;
    MM_HIP(set_device(ws->device));
    if (n_bytes == 0) {
        MM_HIP(hipMemsetAsync(d_counts, 0, 2 * sizeof(uint64_t), ws->stream));
        MM_HIP(hipMemsetAsync(d_rec_base, 0, sizeof(uint64_t), ws->stream));
        if (d_amb) MM_HIP(hipMemsetAsync(d_amb, 0, amb_capacity_bytes < 8 ? amb_capacity_bytes : 8, ws->stream));
        return MM_OK;
    }
    if (!d_text || (!d_packed && packed_capacity_bytes)) return MM_ERR_NULL;
    return MM_PACK_GO_ON;
}

// ... and what their synchronous callers ask of the two counts (bases, records) once they are on the host.
static int pack_counts_check(const uint64_t *out_counts, uint64_t packed_capacity_bytes, uint64_t max_records,
                             const uint8_t *d_amb, uint64_t amb_capacity_bytes) {
    if (out_counts[0] > (packed_capacity_bytes & ~3ull) * 4 || out_counts[1] > max_records) return MM_ERR_CAPACITY;
    if (d_amb && out_counts[0] > amb_capacity_bytes * 8) return MM_ERR_CAPACITY;
    return MM_OK;
}

// (d_amb: the ambiguity bits of mm_fasta_pack_n_*, checked by the caller - always the two-pass kernels; null: the plain packer)
static int fasta_pack_async(mm_workspace_t *ws, const uint8_t *d_text, uint64_t n_bytes,
                            uint8_t *d_packed, uint64_t packed_capacity_bytes, uint64_t *d_rec_base,
                            uint64_t *d_rec_text_pos, uint64_t max_records, uint64_t *d_counts, uint8_t *d_amb,
                            uint64_t amb_capacity_bytes) {
    // (the synchronous wrapper below checks the error word itself; a direct asynchronous caller asks mm_workspace_check)
    const int p = pack_prologue(ws, d_text, n_bytes, d_packed, packed_capacity_bytes, d_rec_base, d_counts, d_amb, amb_capacity_bytes);
    if (p != MM_PACK_GO_ON) return p;
#ifdef MM_EXPERIMENTS
    const uint64_t need_a = mm::fasta_scratch_bytes(n_bytes);
#else
    const uint64_t need_a = 0;
#endif
    const uint64_t need_b = mm::fasta2_scratch_bytes(n_bytes);
    const int r = grow_bytes(ws->scratch, ws->scratch_bytes, need_a > need_b ? need_a : need_b);
    if (r) return r;
    const int choice = d_amb ? 0 : fasta_packer_choice(ws);
    if (choice == 0) {
        if (mm::launch_fasta_pack2(d_text, n_bytes, d_packed, packed_capacity_bytes & ~3ull,
                                   reinterpret_cast<unsigned long long *>(d_rec_base),
                                   reinterpret_cast<unsigned long long *>(d_rec_text_pos), max_records,
                                   reinterpret_cast<unsigned long long *>(d_counts), ws->scratch, ws->stream, d_amb,
                                   amb_capacity_bytes))
            return hip_fail(hipGetLastError(), "fasta_pack2");
        return MM_OK;
    }
#ifndef MM_EXPERIMENTS
    return MM_ERR_HIP;  // (not reached: the product's choice is always 0)
#else
    // The one-pass kernel over lines (mm_fasta.hip: the text read once, one decoupled look-back between 32 KB chunks)
    // was the default since its third version (round 3: 0.96 ms for 1 GiB of 60-base lines against 1.66 ms for the
    // three passes); MM_FASTA_ONEPASS=0 takes the three-pass kernels, which also serve texts the one-pass kernel
    // gives up on (lines shorter than 16 bytes on average - more than 2 048 line segments in a chunk; a look-back
    // time-out).
    const bool one_pass = choice == 1;
    if (one_pass) MM_HIP(hipMemsetAsync(ws->total + 1, 0, sizeof(unsigned long long), ws->stream));
    if (mm::launch_fasta_pack(d_text, n_bytes, d_packed, packed_capacity_bytes & ~3ull,
                              reinterpret_cast<unsigned long long *>(d_rec_base),
                              reinterpret_cast<unsigned long long *>(d_rec_text_pos), max_records,
                              reinterpret_cast<unsigned long long *>(d_counts), ws->scratch, ws->stream, one_pass,
                              error_word(ws)))
        return hip_fail(hipGetLastError(), "fasta_pack");
    return MM_OK;
#endif
}

int mm_fasta_pack_device_async(mm_workspace_t *ws, const uint8_t *d_text, uint64_t n_bytes,
                               uint8_t *d_packed, uint64_t packed_capacity_bytes, uint64_t *d_rec_base,
                               uint64_t *d_rec_text_pos, uint64_t max_records, uint64_t *d_counts) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    return fasta_pack_async(ws, d_text, n_bytes, d_packed, packed_capacity_bytes, d_rec_base, d_rec_text_pos, max_records,
                            d_counts, nullptr, 0);
}

int mm_fasta_pack_n_device_async(mm_workspace_t *ws, const uint8_t *d_text, uint64_t n_bytes,
                                 uint8_t *d_packed, uint64_t packed_capacity_bytes, uint8_t *d_amb,
                                 uint64_t amb_capacity_bytes, uint64_t *d_rec_base, uint64_t *d_rec_text_pos,
                                 uint64_t max_records, uint64_t *d_counts) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    const int c = amb_out_check(d_amb, amb_capacity_bytes);
    if (c) return c;
    return fasta_pack_async(ws, d_text, n_bytes, d_packed, packed_capacity_bytes, d_rec_base, d_rec_text_pos, max_records,
                            d_counts, d_amb, amb_capacity_bytes);
}

// FASTQ (round 4): four-line records, the sequence of every record packed like a FASTA record's (mm_fastq.hip).
// The packer tells a byte's role from the number of newlines in front of it, so the text has to START with its first
// record's '@': `pos_bias` is what a caller that cut blank bytes off the front adds back to the records' text positions.
static int fastq_pack_async(mm_workspace_t *ws, const uint8_t *d_text, uint64_t n_bytes, uint8_t *d_packed,
                            uint64_t packed_capacity_bytes, uint64_t *d_rec_base, uint64_t *d_rec_text_pos,
                            uint64_t max_records, uint64_t *d_counts, uint64_t pos_bias, uint8_t *d_amb,
                            uint64_t amb_capacity_bytes) {
    const int p = pack_prologue(ws, d_text, n_bytes, d_packed, packed_capacity_bytes, d_rec_base, d_counts, d_amb, amb_capacity_bytes);
    if (p != MM_PACK_GO_ON) return p;
    const int r = grow_bytes(ws->scratch, ws->scratch_bytes, mm::fastq_scratch_bytes(n_bytes));
    if (r) return r;
    if (mm::launch_fastq_pack(d_text, n_bytes, d_packed, packed_capacity_bytes & ~3ull,
                              reinterpret_cast<unsigned long long *>(d_rec_base),
                              reinterpret_cast<unsigned long long *>(d_rec_text_pos), max_records,
                              reinterpret_cast<unsigned long long *>(d_counts), ws->scratch, ws->stream, pos_bias, d_amb,
                              amb_capacity_bytes))
        return hip_fail(hipGetLastError(), "fastq_pack");
    return MM_OK;
}

int mm_fastq_pack_device_async(mm_workspace_t *ws, const uint8_t *d_text, uint64_t n_bytes, uint8_t *d_packed,
                               uint64_t packed_capacity_bytes, uint64_t *d_rec_base, uint64_t *d_rec_text_pos,
                               uint64_t max_records, uint64_t *d_counts) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    return fastq_pack_async(ws, d_text, n_bytes, d_packed, packed_capacity_bytes, d_rec_base, d_rec_text_pos, max_records,
                            d_counts, 0, nullptr, 0);
}

int mm_fastq_pack_n_device_async(mm_workspace_t *ws, const uint8_t *d_text, uint64_t n_bytes, uint8_t *d_packed,
                                 uint64_t packed_capacity_bytes, uint8_t *d_amb, uint64_t amb_capacity_bytes,
                                 uint64_t *d_rec_base, uint64_t *d_rec_text_pos, uint64_t max_records, uint64_t *d_counts) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    const int c = amb_out_check(d_amb, amb_capacity_bytes);
    if (c) return c;
    return fastq_pack_async(ws, d_text, n_bytes, d_packed, packed_capacity_bytes, d_rec_base, d_rec_text_pos, max_records,
                            d_counts, 0, d_amb, amb_capacity_bytes);
}

// (d_amb: mm_fasta_pack_n_device, checked by it; null: the plain packers)
static int fasta_pack_sync(mm_workspace_t *ws, const uint8_t *d_text, uint64_t n_bytes, uint8_t *d_packed,
                           uint64_t packed_capacity_bytes, uint64_t *d_rec_base, uint64_t *d_rec_text_pos,
                           uint64_t max_records, uint64_t *d_counts, uint64_t *out_counts, uint8_t *d_amb,
                           uint64_t amb_capacity_bytes) {
    if (!out_counts || !ws) return MM_ERR_NULL;  // (a null workspace used to reach the error branch below)
    // whatever way this call ends, the per-call three-pass flag does not outlive it
    struct ClearOnce {
        mm_workspace_t *w;
        ~ClearOnce() { w->fasta_three_once = false; }
    } clear_once{ws};
    if (d_text && n_bytes) {
        // FASTQ starts with '@' where FASTA starts with '>' (needletail tells them apart the same way)
        unsigned char head[256];
        const size_t nh = n_bytes < sizeof head ? (size_t)n_bytes : sizeof head;
        MM_HIP(set_device(ws->device));
        MM_HIP(hipMemcpyAsync(head, d_text, nh, hipMemcpyDeviceToHost, ws->stream));
        MM_HIP(hipStreamSynchronize(ws->stream));
        size_t i = 0;
        while (i < nh && (head[i] == ' ' || head[i] == '\t' || head[i] == '\r' || head[i] == '\n')) ++i;
        if (i < nh && head[i] == '@') {
            // FASTQ (needletail::parse_fastx tells the formats apart by this byte too): the four-line packer, which
            // counts lines from the start of its text - so it gets the text from the '@' on (blank lines or spaces in
            // front of the first record used to shift every line's role by one: ADVICE r4) and adds the cut back to the
            // records' text positions
            const int r = fastq_pack_async(ws, d_text + i, n_bytes - i, d_packed, packed_capacity_bytes, d_rec_base,
                                           d_rec_text_pos, max_records, d_counts, i, d_amb, amb_capacity_bytes);
            if (r) return r;
            if (d_amb && i) {
                // (the packer cleared what the text behind the cut can fill; the header promises what the whole text can)
                const uint64_t cut = ((n_bytes - i) / 8 + 8 + 3) & ~3ull, whole = (n_bytes / 8 + 8 + 3) & ~3ull;
                const uint64_t from = cut < amb_capacity_bytes ? cut : amb_capacity_bytes;
                const uint64_t to = whole < amb_capacity_bytes ? whole : amb_capacity_bytes;
                if (to > from) MM_HIP(hipMemsetAsync(d_amb + from, 0, to - from, ws->stream));
            }
            MM_HIP(hipMemcpyAsync(out_counts, d_counts, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, ws->stream));
            MM_HIP(hipStreamSynchronize(ws->stream));
            return pack_counts_check(out_counts, packed_capacity_bytes, max_records, d_amb, amb_capacity_bytes);
        }
    }
    for (int attempt = 0; attempt < 2; ++attempt) {
        const int r = fasta_pack_async(ws, d_text, n_bytes, d_packed, packed_capacity_bytes, d_rec_base, d_rec_text_pos,
                                       max_records, d_counts, d_amb, amb_capacity_bytes);
        if (r) return r;
        // (only an attempt that launched the one-pass kernel cleared the error word and may consult it: the three-pass
        // kernels neither clear nor raise it, and a word left by an earlier failed run is not theirs - ADVICE r3)
        const bool was_one_pass = !d_amb && n_bytes != 0 && fasta_packer_choice(ws) == 1;
        MM_HIP(hipMemcpyAsync(out_counts, d_counts, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, ws->stream));
        MM_HIP(hipMemcpyAsync(ws->h_total + 1, ws->total + 1, sizeof(unsigned long long), hipMemcpyDeviceToHost,
                              ws->stream));
        MM_HIP(hipStreamSynchronize(ws->stream));
        if (!was_one_pass || (uint32_t)ws->h_total[1] == 0) break;
        // the one-pass packer gave up: a look-back timed out (chunks not dispatched in order: three passes from now
        // on) or this text's lines are too short for its tables (error 3: three passes for this call)
        if ((uint32_t)ws->h_total[1] == 3u) ws->fasta_three_once = true;
        else ws->fasta_three_pass = true;
        if (!ws->async_unchecked) MM_HIP(hipMemsetAsync(ws->total + 2, 0, sizeof(unsigned long long), ws->stream));
    }
    return pack_counts_check(out_counts, packed_capacity_bytes, max_records, d_amb, amb_capacity_bytes);
}

int mm_fasta_pack_device(mm_workspace_t *ws, const uint8_t *d_text, uint64_t n_bytes, uint8_t *d_packed,
                         uint64_t packed_capacity_bytes, uint64_t *d_rec_base, uint64_t *d_rec_text_pos,
                         uint64_t max_records, uint64_t *d_counts, uint64_t *out_counts) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    return fasta_pack_sync(ws, d_text, n_bytes, d_packed, packed_capacity_bytes, d_rec_base, d_rec_text_pos, max_records,
                           d_counts, out_counts, nullptr, 0);
}

int mm_fasta_pack_n_device(mm_workspace_t *ws, const uint8_t *d_text, uint64_t n_bytes, uint8_t *d_packed,
                           uint64_t packed_capacity_bytes, uint8_t *d_amb, uint64_t amb_capacity_bytes,
                           uint64_t *d_rec_base, uint64_t *d_rec_text_pos, uint64_t max_records, uint64_t *d_counts,
                           uint64_t *out_counts) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    const int c = amb_out_check(d_amb, amb_capacity_bytes);
    if (c) return c;
    return fasta_pack_sync(ws, d_text, n_bytes, d_packed, packed_capacity_bytes, d_rec_base, d_rec_text_pos, max_records,
                           d_counts, out_counts, d_amb, amb_capacity_bytes);
}

// FASTA text -> records of BYTE text (mm_fasta2.hip, fasta2_text_kernel): the reader of mm_fasta_pack_device_async with the
// sequence bytes kept as they are, in the layout mm_run_text_batch_device_async takes.  The packer's checks fit as they
// are (d_seq for d_packed, no ambiguity output); nothing is cleared.
static int fasta_text_async(mm_workspace_t *ws, const uint8_t *d_text, uint64_t n_bytes, uint8_t *d_seq,
                            uint64_t seq_capacity_bytes, uint64_t *d_rec_start, uint64_t *d_rec_text_pos,
                            uint64_t max_records, uint64_t *d_counts) {
    const int p = pack_prologue(ws, d_text, n_bytes, d_seq, seq_capacity_bytes, d_rec_start, d_counts, nullptr, 0);
    if (p != MM_PACK_GO_ON) return p;
    const int r = grow_bytes(ws->scratch, ws->scratch_bytes, mm::fasta2_scratch_bytes(n_bytes));
    if (r) return r;
    if (mm::launch_fasta_text(d_text, n_bytes, d_seq, seq_capacity_bytes, reinterpret_cast<unsigned long long *>(d_rec_start),
                              reinterpret_cast<unsigned long long *>(d_rec_text_pos), max_records,
                              reinterpret_cast<unsigned long long *>(d_counts), ws->scratch, ws->stream))
        return hip_fail(hipGetLastError(), "fasta_text");
    return MM_OK;
}

int mm_fasta_text_device_async(mm_workspace_t *ws, const uint8_t *d_text, uint64_t n_bytes, uint8_t *d_seq,
                               uint64_t seq_capacity_bytes, uint64_t *d_rec_start, uint64_t *d_rec_text_pos,
                               uint64_t max_records, uint64_t *d_counts) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    return fasta_text_async(ws, d_text, n_bytes, d_seq, seq_capacity_bytes, d_rec_start, d_rec_text_pos, max_records, d_counts);
}

int mm_fasta_text_device(mm_workspace_t *ws, const uint8_t *d_text, uint64_t n_bytes, uint8_t *d_seq,
                         uint64_t seq_capacity_bytes, uint64_t *d_rec_start, uint64_t *d_rec_text_pos, uint64_t max_records,
                         uint64_t *d_counts, uint64_t *out_counts) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!out_counts || !ws || !d_counts || !d_rec_start) return MM_ERR_NULL;
    if (n_bytes >= (1ull << 32)) return MM_ERR_LEN_TOO_LARGE;
    if (reinterpret_cast<uintptr_t>(d_seq) % 4 != 0) return MM_ERR_NULL;
    if (d_text && n_bytes) {
        // FASTQ starts with '@' (mm_fasta_pack_device tells the formats apart by this byte too): not read here - a
        // quality line may begin with '>', so the FASTA rules would return nonsense
        unsigned char head[256];
        const size_t nh = n_bytes < sizeof head ? (size_t)n_bytes : sizeof head;
        MM_HIP(set_device(ws->device));
        MM_HIP(hipMemcpyAsync(head, d_text, nh, hipMemcpyDeviceToHost, ws->stream));
        MM_HIP(hipStreamSynchronize(ws->stream));
        size_t i = 0;
        while (i < nh && (head[i] == ' ' || head[i] == '\t' || head[i] == '\r' || head[i] == '\n')) ++i;
        if (i < nh && head[i] == '@') return MM_ERR_FORMAT;
    }
    const int r = fasta_text_async(ws, d_text, n_bytes, d_seq, seq_capacity_bytes, d_rec_start, d_rec_text_pos, max_records,
                                   d_counts);
    if (r) return r;
    MM_HIP(hipMemcpyAsync(out_counts, d_counts, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, ws->stream));
    MM_HIP(hipStreamSynchronize(ws->stream));
    return (out_counts[0] > seq_capacity_bytes || out_counts[1] > max_records) ? MM_ERR_CAPACITY : MM_OK;
}

// The byte-text FASTA kernel's per-thread step on the host (mm_fasta_text.h; no device): the bytes of in[0..32) that
// `mask` selects (bit i = byte i), moved together to out[0..count), zeros behind them; returns the count.
int mm_debug_compact32(const uint8_t in[32], uint32_t mask, uint8_t out[32]) {
    if (!in || !out) return MM_ERR_NULL;
    uint32_t x[8];
    memcpy(x, in, 32);
    const mm::Compact32 c = mm::compact32(x, mask);
    memcpy(out, c.d, 32);
    return (int)c.count;
}

static const uint32_t kProbeGroups = 16;

int mm_clock_probe_begin(mm_workspace_t *ws, uint64_t duration_us) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!ws) return MM_ERR_NULL;
    MM_HIP(set_device(ws->device));
    if (!ws->probe_stream) {
        MM_HIP(hipStreamCreateWithFlags(&ws->probe_stream, hipStreamNonBlocking));
        MM_HIP(hipMalloc(reinterpret_cast<void **>(&ws->probe_out), kProbeGroups * 2 * sizeof(unsigned long long)));
    }
    MM_HIP(hipMemsetAsync(ws->probe_out, 0, kProbeGroups * 2 * sizeof(unsigned long long), ws->probe_stream));
    if (mm::launch_clock_probe(ws->probe_out, kProbeGroups, duration_us * 100ull, ws->probe_stream))
        return hip_fail(hipGetLastError(), "clock_probe");
    return MM_OK;
}

int mm_clock_probe_end(mm_workspace_t *ws, double *ghz) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!ws || !ghz || !ws->probe_stream) return MM_ERR_NULL;
    MM_HIP(set_device(ws->device));
    unsigned long long h[kProbeGroups * 2];
    MM_HIP(hipMemcpyAsync(h, ws->probe_out, sizeof h, hipMemcpyDeviceToHost, ws->probe_stream));
    MM_HIP(hipStreamSynchronize(ws->probe_stream));
    double cyc = 0, real = 0;
    for (uint32_t b = 0; b < kProbeGroups; ++b) {
        cyc += (double)h[2 * b];
        real += (double)h[2 * b + 1];
    }
    *ghz = real > 0 ? cyc / real * 0.1 : 0.0;  // the real-time counter ticks at 100 MHz
    return MM_OK;
}

// Diagnostics: what the host link of this box moves - each direction alone and BOTH AT ONCE (two streams, the copy
// engines), between caller buffers and device memory.  bench.py prints it beside `end_to_end`: the floor of mm_run_host is
// set by the rate at which the two directions run TOGETHER, which is less than the sum of the one-way rates (97 against
// 57.6 + 57.1 GB/s on the boxes of round 5).  out_GBps[0] = host -> device alone, [1] = device -> host alone, [2] = the sum
// of both while they run together.  host_in / host_out: `bytes` each, page-locked for meaningful figures.
int mm_link_probe(mm_workspace_t *ws, const void *host_in, void *host_out, uint64_t bytes, double *out_GBps) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!ws || !host_in || !host_out || !out_GBps || bytes == 0) return MM_ERR_NULL;
    MM_HIP(set_device(ws->device));
    void *d_a = nullptr, *d_b = nullptr;
    hipStream_t s1 = nullptr, s2 = nullptr;
    int rc = MM_OK;
    auto cleanup = [&]() {
        if (s1) hipStreamDestroy(s1);
        if (s2) hipStreamDestroy(s2);
        if (d_a) hipFree(d_a);
        if (d_b) hipFree(d_b);
    };
#define MM_LP(x)                                              \
    do {                                                      \
        const hipError_t e_ = (x);                            \
        if (e_ != hipSuccess) {                               \
            rc = hip_fail(e_, #x);                            \
            cleanup();                                        \
            return rc;                                        \
        }                                                     \
    } while (0)
    MM_LP(hipMalloc(&d_a, bytes));
    MM_LP(hipMalloc(&d_b, bytes));
    MM_LP(hipMemset(d_b, 0, bytes));
    MM_LP(hipStreamCreateWithFlags(&s1, hipStreamNonBlocking));
    MM_LP(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
    // Copies in 32 MiB pieces, at most two per direction in the runtime's hands - the way mm_run_host moves its chunks.
    // (One 512 MiB copy per direction, queued together, measured NO overlap at all inside a process that had loaded
    // another build of the HIP runtime, 57 GB/s for both, where the call itself overlapped them and a stand-alone
    // program measured 97: profiles/r05_host_path.txt.)
    const uint64_t piece = 32ull << 20;
    const uint64_t n_pieces = (bytes + piece - 1) / piece;
    std::vector<hipEvent_t> ev(2 * n_pieces, nullptr);
    auto cleanup_events = [&]() {
        for (hipEvent_t e : ev)
            if (e) hipEventDestroy(e);
    };
    for (hipEvent_t &e : ev)
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
            cleanup_events();
            cleanup();
            return hip_fail(hipGetLastError(), "hipEventCreate");
        }
#define MM_LPE(x)                                             \
    do {                                                      \
        const hipError_t e_ = (x);                            \
        if (e_ != hipSuccess) {                               \
            rc = hip_fail(e_, #x);                            \
            cleanup_events();                                 \
            cleanup();                                        \
            return rc;                                        \
        }                                                     \
    } while (0)
    for (int what = 0; what < 3; ++what) {
        double best = 0.0;
        for (int rep = 0; rep < 4; ++rep) {  // (the first repetition warms up)
            MM_LPE(hipDeviceSynchronize());
            const auto t0 = std::chrono::steady_clock::now();
            uint64_t next[2] = {0, 0}, retired[2] = {0, 0};
            const bool on[2] = {what != 1, what != 0};
            while ((on[0] && retired[0] < n_pieces) || (on[1] && retired[1] < n_pieces)) {
                for (int dir = 0; dir < 2; ++dir) {
                    if (!on[dir]) continue;
                    while (next[dir] < n_pieces && next[dir] - retired[dir] < 2) {
                        const uint64_t o = next[dir] * piece, c = bytes - o < piece ? bytes - o : piece;
                        if (dir == 0)
                            MM_LPE(hipMemcpyAsync(static_cast<uint8_t *>(d_a) + o, static_cast<const uint8_t *>(host_in) + o, c,
                                                  hipMemcpyHostToDevice, s1));
                        else
                            MM_LPE(hipMemcpyAsync(static_cast<uint8_t *>(host_out) + o, static_cast<uint8_t *>(d_b) + o, c,
                                                  hipMemcpyDeviceToHost, s2));
                        MM_LPE(hipEventRecord(ev[2 * next[dir] + dir], dir == 0 ? s1 : s2));
                        ++next[dir];
                    }
                    if (retired[dir] < next[dir]) {
                        const hipError_t q = hipEventQuery(ev[2 * retired[dir] + dir]);
                        if (q == hipSuccess) ++retired[dir];
                        else if (q != hipErrorNotReady) MM_LPE(q);
                        else (void)hipGetLastError();
                    }
                }
            }
            const double t = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            const double rate = (what == 2 ? 2.0 : 1.0) * (double)bytes / t / 1e9;
            if (rep && rate > best) best = rate;
        }
        out_GBps[what] = best;
    }
    cleanup_events();
#undef MM_LPE
#undef MM_LP
    cleanup();
    return MM_OK;
}

int mm_generate_device_async(mm_workspace_t *ws, uint64_t seed, uint64_t first_base,
                             uint64_t n_bases, uint8_t *d_packed) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!ws) return MM_ERR_NULL;
    if (n_bases == 0) return MM_OK;
    if (!d_packed) return MM_ERR_NULL;
    MM_HIP(set_device(ws->device));
    if (mm::launch_generate(seed, first_base, n_bases, d_packed, ws->stream))
        return hip_fail(hipGetLastError(), "generate");
    return MM_OK;
}

// ------------------------------------------------------------------ several devices from one call
// The reference's parallel driver is ordinary host code: rayon over the contigs of a genome, one Builder::run
// per contig (bench/src/bin/paper.rs:442-459).  Here the same call shape for a C / Rust caller: a device group
// holds one workspace per listed device (a device may be listed more than once), and one call fans a sequence
// (window ranges, exact seam) or a set of sequences (greedy longest-first placement) over them - one host
// thread per entry, every shard's positions copied to its place in the caller's single buffer.  The count
// exchange is host-side, so nothing crosses between the devices (no RCCL): results go to host memory.
struct mm_device_group {
    std::vector<mm_workspace_t *> ws;
    // device-resident shards (mm_device_group_upload / _adopt, mm_run_sharded_device)
    std::vector<void *> d_seq;     // the packed sequence as entry i's device addresses it
    std::vector<char> own_seq;     // uploaded by the group (freed with it) / adopted from the caller
    uint64_t seq_bytes = 0;
    // bytes of the sequence that are RESIDENT on entry i ([0, seq_bytes) after _upload / _adopt; the entry's own share
    // plus a halo after mm_device_group_upload_range)
    std::vector<uint64_t> res_lo, res_hi;
    struct Shard {
        uint32_t *d_pos = nullptr, *d_sk = nullptr;  // result buffers on the entry's device, grown as needed
        uint64_t cap_pos = 0, cap_sk = 0;
        uint64_t count = 0, win_begin = 0, win_end = 0;
        bool has_sk = false;
    };
    std::vector<Shard> shard;
    bool ran = false;
    // resident batch (mm_device_group_upload_batch, mm_run_batch_sharded_device): independent sequences placed
    // greedily, longest first, each on its entry's device only
    struct BatchEntry {
        uint8_t *d_buf = nullptr;           // the entry's sequences back to back, each at a 16-byte boundary
        uint64_t buf_bytes = 0;
        std::vector<uint64_t> seqs;         // sequences of this entry, input order
        std::vector<uint64_t> at, nbytes;   // where each lies in d_buf, its packed bytes
        std::vector<uint64_t> offs;         // offsets of its sequences' positions in the entry's result buffer (last run)
        std::vector<uint64_t> run_base, run_len;  // base_offsets / n_bases of its sequences in the last run
        uint64_t *d_vals = nullptr;         // values of the last run's positions (mm_device_group_values_batch), grown as needed
        uint64_t vals_cap = 0;              // ... in 64-bit words
    };
    std::vector<BatchEntry> batch;
    std::vector<int> seq_entry;             // entry of every sequence
    std::vector<uint64_t> seq_slot;         // its index among the entry's sequences
    bool batch_ran = false;
    int batch_vals_words = 0;               // 64-bit words per value in d_vals (1 or 2); 0: no values of the last run
};

namespace {

struct ShardResult {
    int rc = MM_OK;
    std::string err;
    uint64_t count = 0;
};

// Positions [from, from + n) of the workspace's staging buffers to the caller's arrays at `to`.
int copy_shard_out(mm_workspace *ws, uint64_t from, uint64_t n, uint32_t *out_pos, uint32_t *out_sk, uint64_t to) {
    if (n == 0) return MM_OK;
    MM_HIP(hipMemcpyAsync(out_pos + to, ws->d_out + from, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ws->stream));
    if (out_sk)
        MM_HIP(hipMemcpyAsync(out_sk + to, ws->d_sk + from, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ws->stream));
    return MM_OK;
}

}  // namespace

int mm_device_group_create(mm_device_group_t **out, const int *devices, int n_devices) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!out) return MM_ERR_NULL;
    *out = nullptr;
    if (!devices || n_devices <= 0) return MM_ERR_NULL;
    mm_device_group *g = new (std::nothrow) mm_device_group;
    if (!g) return MM_ERR_ALLOC;
    for (int i = 0; i < n_devices; ++i) {
        mm_workspace_t *ws = nullptr;
        const int r = mm_workspace_create(&ws, devices[i], nullptr);
        if (r) {
            mm_device_group_destroy(g);
            return r;
        }
        g->ws.push_back(ws);
    }
    g->d_seq.assign(g->ws.size(), nullptr);
    g->own_seq.assign(g->ws.size(), 0);
    g->shard.resize(g->ws.size());
    // device-to-device copies of mm_device_group_gather go straight over xGMI where the pair allows it (a refusal
    // is not an error: hipMemcpyPeerAsync then stages through the host)
    for (size_t i = 0; i < g->ws.size(); ++i)
        for (size_t j = 0; j < g->ws.size(); ++j)
            if (g->ws[i]->device != g->ws[j]->device) {
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, g->ws[i]->device, g->ws[j]->device) == hipSuccess && can &&
                    set_device(g->ws[i]->device) == hipSuccess)
                    (void)hipDeviceEnablePeerAccess(g->ws[j]->device, 0);
                (void)hipGetLastError();
            }
    *out = g;
    return MM_OK;
}

static void group_drop_sequence(mm_device_group *g) {
    for (size_t i = 0; i < g->d_seq.size(); ++i)
        if (g->d_seq[i] && g->own_seq[i]) {
            set_device(g->ws[i]->device);
            hipFree(g->d_seq[i]);
        }
    g->d_seq.assign(g->ws.size(), nullptr);
    g->own_seq.assign(g->ws.size(), 0);
    g->res_lo.assign(g->ws.size(), 0);
    g->res_hi.assign(g->ws.size(), 0);
    g->seq_bytes = 0;
}

void mm_device_group_destroy(mm_device_group_t *g) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!g) return;
    for (size_t i = 0; i < g->shard.size() && i < g->ws.size(); ++i) {
        set_device(g->ws[i]->device);
        hipStreamSynchronize(g->ws[i]->stream);
        if (g->shard[i].d_pos) hipFree(g->shard[i].d_pos);
        if (g->shard[i].d_sk) hipFree(g->shard[i].d_sk);
    }
    if (!g->d_seq.empty()) group_drop_sequence(g);
    for (size_t i = 0; i < g->batch.size() && i < g->ws.size(); ++i)
        if (g->batch[i].d_buf || g->batch[i].d_vals) {
            set_device(g->ws[i]->device);
            if (g->batch[i].d_buf) hipFree(g->batch[i].d_buf);
            if (g->batch[i].d_vals) hipFree(g->batch[i].d_vals);
        }
    for (mm_workspace_t *ws : g->ws) mm_workspace_destroy(ws);
    delete g;
}

int mm_device_group_upload(mm_device_group_t *g, const uint8_t *packed, uint64_t packed_bytes) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!g || g->ws.empty() || !packed || packed_bytes == 0) return MM_ERR_NULL;
    group_drop_sequence(g);
    // (+ 64 bytes of zeros: the walk's loads run a few dwords ahead of the last base)
    for (size_t i = 0; i < g->ws.size(); ++i) {
        MM_HIP(set_device(g->ws[i]->device));
        void *p = nullptr;
        hipError_t e = hipMalloc(&p, packed_bytes + 64);
        if (e != hipSuccess) {
            g_last_error = std::string("hipMalloc: ") + hipGetErrorString(e);
            group_drop_sequence(g);
            return MM_ERR_ALLOC;
        }
        g->d_seq[i] = p;
        g->own_seq[i] = 1;
        // all copies in flight together (page-locked sources copy asynchronously; pageable ones serialise)
        MM_HIP(hipMemsetAsync(static_cast<uint8_t *>(p) + packed_bytes, 0, 64, g->ws[i]->stream));
        MM_HIP(hipMemcpyAsync(p, packed, packed_bytes, hipMemcpyHostToDevice, g->ws[i]->stream));
    }
    for (size_t i = 0; i < g->ws.size(); ++i) {
        MM_HIP(set_device(g->ws[i]->device));
        MM_HIP(hipStreamSynchronize(g->ws[i]->stream));
    }
    g->seq_bytes = packed_bytes;
    g->res_hi.assign(g->ws.size(), packed_bytes);
    return MM_OK;
}


// The bytes entry i of an N-way window split can read, for ANY plan (k + w - 1 below 2^17): its share of the bases,
// the largest window in front and behind, a lane's over-read behind a range (the walk of a lane that starts inside the
// range runs its whole length: below 60 000 bases) and the look-ahead of the loads.
static void resident_range(uint64_t base_offset, uint64_t n_bases, uint64_t N, uint64_t i, uint64_t total_bytes, uint64_t *lo,
                           uint64_t *hi) {
    const uint64_t kMaxL = 1ull << 17, kOver = 4ull * mm::fused_overread_bytes();  // (bases)
    const uint64_t nb_lo = n_bases > kMaxL ? n_bases - kMaxL : 0;
    uint64_t first = base_offset + nb_lo / N * i;
    first = first / 4 > 64 ? first / 4 - 64 : 0;
    *lo = first & ~255ull;
    const uint64_t last = (base_offset + n_bases / N * (i + 1) + n_bases % N + kMaxL + kOver) / 4 + 4096;
    *hi = (i + 1 == N || last > total_bytes) ? total_bytes : last;
}

int mm_device_group_upload_range(mm_device_group_t *g, const uint8_t *packed, uint64_t packed_bytes, uint64_t base_offset,
                                 uint64_t n_bases) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!g || g->ws.empty() || !packed || packed_bytes == 0) return MM_ERR_NULL;
    if ((base_offset + n_bases + 3) / 4 > packed_bytes) return MM_ERR_CAPACITY;
    group_drop_sequence(g);
    const uint64_t N = g->ws.size();
    for (uint64_t i = 0; i < N; ++i) {
        MM_HIP(set_device(g->ws[i]->device));
        void *p = nullptr;
        // (the whole extent is ALLOCATED on every device so that offsets stay absolute; only the entry's range crosses
        // the host link.  What is not uploaded is filled with a pattern: a run can never depend on stale memory.)
        hipError_t e = hipMalloc(&p, packed_bytes + 64);
        if (e != hipSuccess) {
            g_last_error = std::string("hipMalloc: ") + hipGetErrorString(e);
            group_drop_sequence(g);
            return MM_ERR_ALLOC;
        }
        g->d_seq[i] = p;
        g->own_seq[i] = 1;
        uint64_t lo, hi;
        resident_range(base_offset, n_bases, N, i, packed_bytes, &lo, &hi);
        g->res_lo[i] = lo;
        g->res_hi[i] = hi;
        uint8_t *d = static_cast<uint8_t *>(p);
        if (lo) MM_HIP(hipMemsetAsync(d, 0xA5, lo, g->ws[i]->stream));
        if (hi < packed_bytes) MM_HIP(hipMemsetAsync(d + hi, 0xA5, packed_bytes - hi, g->ws[i]->stream));
        MM_HIP(hipMemsetAsync(d + packed_bytes, 0, 64, g->ws[i]->stream));
        MM_HIP(hipMemcpyAsync(d + lo, packed + lo, hi - lo, hipMemcpyHostToDevice, g->ws[i]->stream));
    }
    for (uint64_t i = 0; i < N; ++i) {
        MM_HIP(set_device(g->ws[i]->device));
        MM_HIP(hipStreamSynchronize(g->ws[i]->stream));
    }
    g->seq_bytes = packed_bytes;
    return MM_OK;
}

int mm_device_group_adopt(mm_device_group_t *g, const void *const *d_packed, uint64_t packed_bytes) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!g || g->ws.empty() || !d_packed || packed_bytes == 0) return MM_ERR_NULL;
    for (size_t i = 0; i < g->ws.size(); ++i)
        if (!d_packed[i]) return MM_ERR_NULL;
    group_drop_sequence(g);
    for (size_t i = 0; i < g->ws.size(); ++i) g->d_seq[i] = const_cast<void *>(d_packed[i]);
    g->res_hi.assign(g->ws.size(), packed_bytes);
    g->seq_bytes = packed_bytes;
    return MM_OK;
}

int mm_device_group_size(const mm_device_group_t *g) { return g ? (int)g->ws.size() : 0; }

int mm_run_sharded_host(const mm_plan_t *plan, mm_device_group_t *g, const uint8_t *packed, uint64_t base_offset,
                        uint64_t n_bases, uint32_t *out_pos, uint32_t *out_sk, uint64_t capacity,
                        uint64_t *out_count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (const int bad = dna_plan_only(plan)) return bad;
    if (!plan || !g || g->ws.empty()) return MM_ERR_NULL;
    if (n_bases >= (1ull << 32)) return MM_ERR_LEN_TOO_LARGE;
    if (out_sk && plan->mode != MM_MINIMIZERS) return MM_ERR_BAD_MODE;
    if (out_count) *out_count = 0;
    const uint64_t l = (uint64_t)plan->k + plan->w - 1;
    const uint64_t n_w = n_bases >= l ? n_bases - l + 1 : 0;
    if (n_w == 0) return MM_OK;
    if (!packed) return MM_ERR_NULL;
    const uint64_t N = g->ws.size();
    const uint64_t bytes = (base_offset + n_bases + 3) / 4;
    std::vector<ShardResult> res(N);
    std::vector<uint64_t> wb(N + 1);
    for (uint64_t i = 0; i <= N; ++i) wb[i] = n_w / N * i + (n_w % N) * i / N;  // equal window ranges
    wb[N] = n_w;
    // ---- phase 1: every shard uploads the bytes its windows read, runs, reports count / first / last
    auto phase1 = [&](uint64_t i) {
        ShardResult &r = res[i];
        mm_workspace *ws = g->ws[i];
        const uint64_t a = wb[i], e = wb[i + 1];
        if (a >= e) return;
        auto fail = [&](int rc) {
            r.rc = rc;
            r.err = g_last_error;
        };
        if (set_device(ws->device) != hipSuccess) return fail(MM_ERR_HIP);
        // (the whole extent, so that positions stay absolute; only this shard's slice of it is filled)
        int rc = grow_bytes(ws->d_in, ws->d_in_bytes, bytes + 16);
        if (rc) return fail(rc);
        uint8_t *const din = static_cast<uint8_t *>(ws->d_in);
        // element 0 of the first lane is the k-mer before window a; the walk's loads run a few dwords ahead
        const uint64_t b0 = a ? ((base_offset + a - 1) / 4) & ~15ull : 0;
        uint64_t b1 = (base_offset + e + l - 2) / 4 + 1 + 64 + plan->w / 2;
        if (b1 > bytes) b1 = bytes;
        if (hipMemcpyAsync(din + b0, packed + b0, b1 - b0, hipMemcpyHostToDevice, ws->stream) != hipSuccess)
            return fail(MM_ERR_HIP);
        const uint64_t cap = (e - a) < capacity ? (e - a) : capacity;
        rc = grow(ws->d_out, ws->d_out_elems, cap ? cap : 1, sizeof(uint32_t));
        if (rc == MM_OK && out_sk) rc = grow(ws->d_sk, ws->d_sk_elems, cap ? cap : 1, sizeof(uint32_t));
        if (rc) return fail(rc);
        uint64_t count = 0;
        rc = run_device_sync(plan, ws, {.d_packed = ws->d_in, .packed_bytes = bytes + 16, .base_offset = base_offset,
                                        .n_bases = n_bases, .win_begin = a, .win_end = e, .d_out_pos = out_pos ? ws->d_out : nullptr,
                                        .d_out_sk = (out_sk && out_pos) ? ws->d_sk : nullptr, .capacity = out_pos ? cap : 0},
                             &count);
        r.count = count;
        if (rc && rc != MM_ERR_CAPACITY) return fail(rc);
        if (rc == MM_ERR_CAPACITY) r.rc = rc;
    };
    {
        std::vector<std::thread> th;
        for (uint64_t i = 1; i < N; ++i) th.emplace_back(phase1, i);
        phase1(0);
        for (std::thread &t : th) t.join();
    }
    for (uint64_t i = 0; i < N; ++i)
        if (res[i].rc && res[i].rc != MM_ERR_CAPACITY) {
            g_last_error = res[i].err;
            return res[i].rc;
        }
    // ---- the seam between consecutive shards needs nothing here: the reference drops a lane's first position when
    // it equals the last one before it (src/collect.rs:265-271), and a window-range run already starts by comparing
    // with the window BEFORE its range (element 0 of its first lane), so a shard never begins with a repeat.  (Rounds
    // 1-3 read every shard's first and last position back to apply a rule that could not fire.)
    std::vector<uint64_t> drop(N, 0), off(N + 1, 0);
    bool over = false;
    for (uint64_t i = 0; i < N; ++i) {
        if (res[i].rc == MM_ERR_CAPACITY) over = true;
        off[i + 1] = off[i] + res[i].count;
    }
    if (out_count) *out_count = off[N];
    if (over || (out_pos && off[N] > capacity)) return MM_ERR_CAPACITY;
    if (!out_pos) return MM_OK;
    // ---- phase 2: every shard's positions to their place in the caller's buffer
    auto phase2 = [&](uint64_t i) {
        mm_workspace *ws = g->ws[i];
        if (res[i].count <= drop[i]) return;
        if (set_device(ws->device) != hipSuccess ||
            copy_shard_out(ws, drop[i], res[i].count - drop[i], out_pos, out_sk, off[i]) != MM_OK ||
            hipStreamSynchronize(ws->stream) != hipSuccess) {
            res[i].rc = MM_ERR_HIP;
            res[i].err = g_last_error;
        }
    };
    {
        std::vector<std::thread> th;
        for (uint64_t i = 1; i < N; ++i) th.emplace_back(phase2, i);
        phase2(0);
        for (std::thread &t : th) t.join();
    }
    for (uint64_t i = 0; i < N; ++i)
        if (res[i].rc) {
            g_last_error = res[i].err;
            return res[i].rc;
        }
    return MM_OK;
}

// ---- device-resident shards: one asynchronous launch per entry from the calling thread, results stay on the devices
int mm_run_sharded_device(const mm_plan_t *plan, mm_device_group_t *g, uint64_t base_offset, uint64_t n_bases,
                          int want_superkmers, uint64_t *counts, uint64_t *total) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (const int bad = dna_plan_only(plan)) return bad;
    if (!plan || !g || g->ws.empty()) return MM_ERR_NULL;
    if (g->seq_bytes == 0) {
        g_last_error = "mm_run_sharded_device: no resident sequence (mm_device_group_upload / _adopt first)";
        return MM_ERR_NULL;
    }
    if (n_bases >= (1ull << 32)) return MM_ERR_LEN_TOO_LARGE;
    if (want_superkmers && plan->mode != MM_MINIMIZERS) return MM_ERR_BAD_MODE;  // src/lib.rs:339
    if ((base_offset + n_bases + 3) / 4 > g->seq_bytes) return MM_ERR_CAPACITY;
    const uint64_t N = g->ws.size();
    const uint64_t l = (uint64_t)plan->k + plan->w - 1;
    const uint64_t n_w = n_bases >= l ? n_bases - l + 1 : 0;
    if (total) *total = 0;
    g->ran = true;
    g->batch_ran = false;  // (the result buffers are shared between the two resident modes: ADVICE r4)
    g->batch_vals_words = 0;
    // expected positions per window (+ 15 % and a constant): a shard that needs more is run again with what it needs
    const double dens = expected_density(plan);
    std::vector<char> host_written(N, 0), pending(N, 0);
    auto grow_shard = [&](uint64_t i, uint64_t need) -> int {
        mm_device_group::Shard &s = g->shard[i];
        int r = grow(s.d_pos, s.cap_pos, need ? need : 1, sizeof(uint32_t));
        if (r == MM_OK && want_superkmers) r = grow(s.d_sk, s.cap_sk, need ? need : 1, sizeof(uint32_t));
        return r;
    };
    auto issue = [&](uint64_t i) -> int {
        mm_device_group::Shard &s = g->shard[i];
        mm_workspace *ws = g->ws[i];
        MM_HIP(set_device(ws->device));
        bool hw = false;
        ws->h_total[0] = 0;
        ws->h_total[1] = 0;
        if (!ws->h_total_dev) MM_HIP(hipMemsetAsync(ws->total + 1, 0, sizeof(unsigned long long), ws->stream));
        const uint64_t cap = want_superkmers ? (s.cap_pos < s.cap_sk ? s.cap_pos : s.cap_sk) : s.cap_pos;
        int r = run_device_async_impl(plan, ws, {.d_packed = g->d_seq[i], .packed_bytes = g->seq_bytes + (g->own_seq[i] ? 64 : 0),
                                                 .base_offset = base_offset, .n_bases = n_bases, .win_begin = s.win_begin,
                                                 .win_end = s.win_end, .d_out_pos = s.d_pos,
                                                 .d_out_sk = want_superkmers ? s.d_sk : nullptr, .capacity = cap,
                                                 .host_total_written = &hw});
        if (r) return r;
        if (!hw)
            MM_HIP(hipMemcpyAsync(ws->h_total, ws->total, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                  ws->stream));
        host_written[i] = hw ? 1 : 0;
        pending[i] = 1;
        return MM_OK;
    };
    for (uint64_t i = 0; i < N; ++i) {
        mm_device_group::Shard &s = g->shard[i];
        s.win_begin = n_w / N * i + (n_w % N) * i / N;  // equal window ranges
        s.win_end = i + 1 == N ? n_w : n_w / N * (i + 1) + (n_w % N) * (i + 1) / N;
        s.count = 0;
        s.has_sk = want_superkmers != 0;
        if (s.win_begin >= s.win_end) continue;
        {   // what this entry's run reads must be resident on it (mm_device_group_upload_range uploads a share + halo)
            const uint64_t lw = (uint64_t)plan->k + plan->w - 1;
            const uint64_t need_lo = (base_offset + (s.win_begin ? s.win_begin - 1 : 0)) / 4;
            // (+ what the launch may touch behind its last window: the launcher's own bound, mm_launch.h)
            uint64_t need_hi = (base_offset + s.win_end + lw - 2) / 4 + 1 + mm::fused_overread_bytes();
            if (need_hi > g->seq_bytes) need_hi = g->seq_bytes;
            if (need_lo < g->res_lo[i] || need_hi > g->res_hi[i]) {
                g_last_error = "mm_run_sharded_device: entry " + std::to_string(i) + " holds bytes [" + std::to_string(g->res_lo[i]) +
                               ", " + std::to_string(g->res_hi[i]) + ") of the sequence, this run reads [" + std::to_string(need_lo) +
                               ", " + std::to_string(need_hi) + "): upload the range this run covers (mm_device_group_upload_range) "
                               "or the whole sequence (mm_device_group_upload)";
                return MM_ERR_NULL;
            }
        }
        const uint64_t nw = s.win_end - s.win_begin;
        uint64_t want = (uint64_t)(dens * 1.15 * (double)nw) + 4096;
        if (want > nw) want = nw;
        MM_HIP(set_device(g->ws[i]->device));
        int r = grow_shard(i, want);
        if (r) return r;
        r = issue(i);
        if (r) return r;
    }
    // wait for the shards in turn; a shard that reports a look-back time-out or needs more room runs again
    uint64_t sum = 0;
    for (uint64_t i = 0; i < N; ++i) {
        mm_device_group::Shard &s = g->shard[i];
        mm_workspace *ws = g->ws[i];
        for (int attempt = 0; pending[i] && attempt < 4; ++attempt) {
            MM_HIP(set_device(ws->device));
            MM_HIP(hipStreamSynchronize(ws->stream));
            pending[i] = 0;
            const int je = judge_run_error(ws);
            if (je < 0) return je;
            const uint64_t cnt = ws->h_total[0];
            const uint64_t cap = want_superkmers ? (s.cap_pos < s.cap_sk ? s.cap_pos : s.cap_sk) : s.cap_pos;
            if (je == 1 || cnt > cap) {  // ticket mode is now on / the true count is known
                if (cnt > cap) {
                    const int r = grow_shard(i, cnt);
                    if (r) return r;
                }
                const int r = issue(i);
                if (r) return r;
                continue;
            }
            s.count = cnt;
        }
        if (pending[i]) {
            g_last_error = "mm_run_sharded_device: a shard did not complete";
            return MM_ERR_HIP;
        }
        if (counts) counts[i] = s.count;
        sum += s.count;
    }
    if (total) *total = sum;
    return MM_OK;
}

int mm_device_group_result(const mm_device_group_t *g, int entry, uint32_t **d_pos, uint32_t **d_sk, uint64_t *count,
                           uint64_t *win_begin, uint64_t *win_end) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!g || entry < 0 || (size_t)entry >= g->shard.size() || !g->ran) return MM_ERR_NULL;
    const mm_device_group::Shard &s = g->shard[(size_t)entry];
    if (d_pos) *d_pos = s.d_pos;
    if (d_sk) *d_sk = s.has_sk ? s.d_sk : nullptr;
    if (count) *count = s.count;
    if (win_begin) *win_begin = s.win_begin;
    if (win_end) *win_end = s.win_end;
    return MM_OK;
}

int mm_device_group_gather(mm_device_group_t *g, int root, uint32_t *d_dst_pos, uint32_t *d_dst_sk, uint64_t capacity,
                           uint64_t *total) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!g || root < 0 || (size_t)root >= g->ws.size() || !g->ran) return MM_ERR_NULL;
    uint64_t sum = 0;
    for (const mm_device_group::Shard &s : g->shard) sum += s.count;
    if (total) *total = sum;
    if (sum > capacity) return MM_ERR_CAPACITY;
    if (sum && !d_dst_pos) return MM_ERR_NULL;
    const int root_dev = g->ws[(size_t)root]->device;
    uint64_t off = 0;
    for (size_t i = 0; i < g->ws.size(); ++i) {
        const mm_device_group::Shard &s = g->shard[i];
        mm_workspace *ws = g->ws[i];
        if (s.count) {
            if (d_dst_sk && !s.has_sk) return MM_ERR_BAD_MODE;
            // every copy on its SOURCE entry's stream: all of them in flight together, one link each
            MM_HIP(set_device(ws->device));
            MM_HIP(hipMemcpyPeerAsync(d_dst_pos + off, root_dev, s.d_pos, ws->device, s.count * sizeof(uint32_t), ws->stream));
            if (d_dst_sk)
                MM_HIP(hipMemcpyPeerAsync(d_dst_sk + off, root_dev, s.d_sk, ws->device, s.count * sizeof(uint32_t), ws->stream));
        }
        off += s.count;
    }
    for (size_t i = 0; i < g->ws.size(); ++i) {
        MM_HIP(set_device(g->ws[i]->device));
        MM_HIP(hipStreamSynchronize(g->ws[i]->stream));
    }
    return MM_OK;
}

// ---- device-resident batches: independent sequences (contigs), each on ONE device of the group
int mm_device_group_upload_batch(mm_device_group_t *g, uint64_t n_seqs, const uint8_t *const *packed,
                                 const uint64_t *packed_bytes) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!g || g->ws.empty() || (n_seqs && (!packed || !packed_bytes))) return MM_ERR_NULL;
    const uint64_t N = g->ws.size();
    // greedy placement, longest sequence first onto the least loaded entry (sharding.assign_contigs)
    std::vector<uint64_t> order(n_seqs);
    for (uint64_t s = 0; s < n_seqs; ++s) order[s] = s;
    std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return packed_bytes[a] > packed_bytes[b]; });
    std::vector<uint64_t> load(N, 0);
    g->batch.resize(N);
    for (mm_device_group::BatchEntry &b : g->batch) {
        b.seqs.clear();
        b.at.clear();
        b.nbytes.clear();
        b.offs.clear();
    }
    g->seq_entry.assign(n_seqs, 0);
    g->seq_slot.assign(n_seqs, 0);
    g->batch_ran = false;
    g->batch_vals_words = 0;
    for (uint64_t s : order) {
        uint64_t best = 0;
        for (uint64_t i = 1; i < N; ++i)
            if (load[i] < load[best]) best = i;
        g->batch[best].seqs.push_back(s);
        load[best] += packed_bytes[s];
    }
    for (uint64_t i = 0; i < N; ++i) {
        mm_device_group::BatchEntry &b = g->batch[i];
        std::sort(b.seqs.begin(), b.seqs.end());
        uint64_t total = 0;
        for (size_t j = 0; j < b.seqs.size(); ++j) {
            const uint64_t s = b.seqs[j];
            g->seq_entry[s] = (int)i;
            g->seq_slot[s] = j;
            b.at.push_back(total);
            b.nbytes.push_back(packed_bytes[s]);
            total += (packed_bytes[s] + 64 + 15) & ~15ull;  // (the walk's loads run a few dwords past the last base)
        }
        MM_HIP(set_device(g->ws[i]->device));
        int r = grow(b.d_buf, b.buf_bytes, total + 16, 1);
        if (r) return r;
        MM_HIP(hipMemsetAsync(b.d_buf, 0, b.buf_bytes, g->ws[i]->stream));
        for (size_t j = 0; j < b.seqs.size(); ++j)
            if (b.nbytes[j]) {
                if (!packed[b.seqs[j]]) return MM_ERR_NULL;
                MM_HIP(hipMemcpyAsync(b.d_buf + b.at[j], packed[b.seqs[j]], b.nbytes[j], hipMemcpyHostToDevice, g->ws[i]->stream));
            }
    }
    for (uint64_t i = 0; i < N; ++i) {
        MM_HIP(set_device(g->ws[i]->device));
        MM_HIP(hipStreamSynchronize(g->ws[i]->stream));
    }
    return MM_OK;
}

int mm_run_batch_sharded_device(const mm_plan_t *plan, mm_device_group_t *g, const uint64_t *base_offsets,
                                const uint64_t *n_bases, int want_superkmers, uint64_t *out_counts, uint64_t *total) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (const int bad = dna_plan_only(plan)) return bad;
    if (!plan || !g || g->ws.empty() || g->batch.size() != g->ws.size() || !n_bases) return MM_ERR_NULL;
    if (want_superkmers && plan->mode != MM_MINIMIZERS) return MM_ERR_BAD_MODE;
    const uint64_t N = g->ws.size(), n_seqs = g->seq_entry.size();
    const uint64_t l = (uint64_t)plan->k + plan->w - 1;
    const double dens = expected_density(plan);
    // One batch launch per entry, ISSUED from this thread one after the other (nothing waits), then waited for in
    // turn - the model of mm_run_sharded_device (round 4 ran a host thread per entry here because a batch launch read
    // its offsets back synchronously; round 5 split it into batch_issue / batch_finish).  An entry whose plan has no
    // fused kernel, whose lists time out or whose results need more room than the expected density is run again,
    // alone and synchronously, when its turn to be waited for comes.
    struct Entry {
        std::vector<const void *> dptr;
        std::vector<uint64_t> dbytes, offs, lens;
        BatchIssue bi;
        uint64_t want = 0;
        bool issued = false, sync_path = false;
    };
    std::vector<Entry> ent(N);
    g->ran = false;  // (the result buffers now hold a batch: mm_device_group_result / _gather must not read them as shards)
    g->batch_ran = false;
    g->batch_vals_words = 0;
    // (an error on a later entry must not leave the earlier entries' launches - and their uploads out of `ent`'s
    // host vectors - in flight when `ent` is destroyed: every issued entry is waited for and its error words consumed
    // before the first error is returned)
    auto drain = [&](int code) -> int {
        for (uint64_t i = 0; i < N; ++i) {
            if (!ent[i].issued) continue;
            if (set_device(g->ws[i]->device) == hipSuccess) {
                (void)hipStreamSynchronize(g->ws[i]->stream);
                (void)judge_run_error(g->ws[i]);
            }
            (void)hipGetLastError();
            ent[i].issued = false;
        }
        return code;
    };
    const int rc_all = [&]() -> int {
    auto grow_entry = [&](uint64_t i, uint64_t want) -> int {
        mm_device_group::Shard &sh = g->shard[i];
        int rc = grow(sh.d_pos, sh.cap_pos, want ? want : 1, sizeof(uint32_t));
        if (rc == MM_OK && want_superkmers) rc = grow(sh.d_sk, sh.cap_sk, want ? want : 1, sizeof(uint32_t));
        return rc;
    };
    auto cap_of = [&](uint64_t i) -> uint64_t {
        const mm_device_group::Shard &sh = g->shard[i];
        return want_superkmers ? (sh.cap_pos < sh.cap_sk ? sh.cap_pos : sh.cap_sk) : sh.cap_pos;
    };
    for (uint64_t i = 0; i < N; ++i) {
        mm_device_group::BatchEntry &b = g->batch[i];
        mm_device_group::Shard &sh = g->shard[i];
        Entry &e = ent[i];
        sh.count = 0;
        sh.has_sk = want_superkmers != 0;
        b.offs.assign(b.seqs.size() + 1, 0);
        if (b.seqs.empty()) continue;
        MM_HIP(set_device(g->ws[i]->device));
        const size_t m = b.seqs.size();
        e.dptr.resize(m);
        e.dbytes.resize(m);
        e.offs.resize(m);
        e.lens.resize(m);
        uint64_t windows = 0;
        for (size_t j = 0; j < m; ++j) {
            const uint64_t s = b.seqs[j];
            e.offs[j] = base_offsets ? base_offsets[s] : 0;
            e.lens[j] = n_bases[s];
            if ((e.offs[j] + e.lens[j] + 3) / 4 > b.nbytes[j]) return MM_ERR_CAPACITY;  // more bases than were uploaded
            e.dptr[j] = b.d_buf + b.at[j];
            e.dbytes[j] = b.nbytes[j] + 64;
            windows += e.lens[j] >= l ? e.lens[j] - l + 1 : 0;
        }
        e.want = (uint64_t)(dens * 1.15 * (double)windows) + 4096;
        if (e.want > windows) e.want = windows;
        int rc = grow_entry(i, e.want);
        if (rc) return rc;
        rc = batch_issue(plan, g->ws[i], {.n_seqs = m, .d_packed = e.dptr.data(), .packed_bytes = e.dbytes.data(),
                                          .base_offsets = e.offs.data(), .n_bases = e.lens.data(), .d_out_pos = sh.d_pos,
                                          .d_out_sk = want_superkmers ? sh.d_sk : nullptr, .capacity = cap_of(i)}, &e.bi);
        if (rc == MM_BATCH_FALLBACK) e.sync_path = true;  // (no fused kernel for this plan: the per-sequence loop, below)
        else if (rc) return rc;
        else e.issued = true;
    }
    for (uint64_t i = 0; i < N; ++i) {
        mm_device_group::BatchEntry &b = g->batch[i];
        mm_device_group::Shard &sh = g->shard[i];
        Entry &e = ent[i];
        if (b.seqs.empty()) continue;
        MM_HIP(set_device(g->ws[i]->device));
        const size_t m = b.seqs.size();
        int rc = MM_OK;
        if (e.issued) {
            rc = batch_finish(g->ws[i], &e.bi, true, cap_of(i), b.offs.data());
            e.issued = rc == MM_ERR_HIP;  // (anything but a failed wait: the entry's launch is over and its words are judged)
            if (rc == MM_BATCH_REDO) e.sync_path = true;
            else if (rc == MM_ERR_CAPACITY) {  // denser than expected: again with what it needs
                e.want = b.offs[m];
                e.sync_path = true;
            } else if (rc) return rc;
        }
        for (int attempt = 0; e.sync_path && attempt < 2; ++attempt) {
            rc = grow_entry(i, e.want);
            if (rc) return rc;
            rc = mm_run_batch_device(plan, g->ws[i], m, e.dptr.data(), e.dbytes.data(), e.offs.data(), e.lens.data(), sh.d_pos,
                                     want_superkmers ? sh.d_sk : nullptr, cap_of(i), b.offs.data());
            if (rc == MM_ERR_CAPACITY && attempt == 0) {
                e.want = b.offs[m];
                continue;
            }
            if (rc) return rc;
            break;
        }
        sh.count = b.offs[m];
        e.issued = false;  // (waited for and judged)
    }
    return MM_OK;
    }();
    if (rc_all) return drain(rc_all);
    uint64_t sum = 0;
    for (uint64_t s = 0; s < n_seqs; ++s) {
        const mm_device_group::BatchEntry &b = g->batch[(size_t)g->seq_entry[s]];
        const uint64_t c = b.offs[g->seq_slot[s] + 1] - b.offs[g->seq_slot[s]];
        if (out_counts) out_counts[s] = c;
        sum += c;
    }
    if (total) *total = sum;
    // (what mm_device_group_values_batch needs of this run: where every sequence's first base lies and how many follow)
    for (uint64_t i = 0; i < N; ++i) {
        g->batch[i].run_base = ent[i].offs;
        g->batch[i].run_len = ent[i].lens;
    }
    g->batch_ran = true;
    return MM_OK;
}

int mm_device_group_batch_result(const mm_device_group_t *g, uint64_t seq, int *entry, uint32_t **d_pos, uint32_t **d_sk,
                                 uint64_t *count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!g || !g->batch_ran || seq >= g->seq_entry.size()) return MM_ERR_NULL;
    const int e = g->seq_entry[seq];
    const mm_device_group::BatchEntry &b = g->batch[(size_t)e];
    const mm_device_group::Shard &sh = g->shard[(size_t)e];
    const uint64_t j = g->seq_slot[seq];
    if (entry) *entry = e;
    if (d_pos) *d_pos = sh.d_pos ? sh.d_pos + b.offs[j] : nullptr;
    if (d_sk) *d_sk = (sh.has_sk && sh.d_sk) ? sh.d_sk + b.offs[j] : nullptr;
    if (count) *count = b.offs[j + 1] - b.offs[j];
    return MM_OK;
}

// ---- Output::values_u64 / values_u128 (src/lib.rs:584-629) of the last batch run's positions, per entry in ONE launch of
// the batch values kernel over the entry's resident sequences (what a loop over the contigs, bench/src/bin/paper.rs:410-431,
// would ask of Output::values_* one by one).  Issued from this thread one entry after the other, then waited for.
int mm_device_group_values_batch(mm_device_group_t *g, uint32_t len, int canonical, int want_u128, uint64_t *total) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!g || !g->batch_ran || g->batch.size() != g->ws.size()) return MM_ERR_NULL;
    if (len == 0 || len > (want_u128 ? 64u : 32u)) return MM_ERR_VALUE_LEN;
    const uint64_t N = g->ws.size(), words = want_u128 ? 2 : 1;
    g->batch_vals_words = 0;
    uint64_t sum = 0;
    int rc = MM_OK;
    for (uint64_t i = 0; i < N && rc == MM_OK; ++i) {
        mm_device_group::BatchEntry &b = g->batch[i];
        const size_t m = b.seqs.size();
        const uint64_t count = m ? b.offs[m] : 0;
        if (count == 0) continue;
        if (b.run_base.size() != m || b.run_len.size() != m) {
            rc = MM_ERR_NULL;
            break;
        }
        if (set_device(g->ws[i]->device) != hipSuccess) {
            rc = hip_fail(hipGetLastError(), "hipSetDevice");
            break;
        }
        rc = grow(b.d_vals, b.vals_cap, words * count, sizeof(uint64_t));
        if (rc) break;
        // the sequences as they lie in the entry's buffer, with the bytes that were uploaded for each (the zeros the upload
        // put behind them are what a position past a sequence's end reads anyway)
        std::vector<const void *> dptr(m);
        for (size_t j = 0; j < m; ++j) dptr[j] = b.d_buf + b.at[j];
        // (the tables are copied into the workspace's page-locked area before the call returns: dptr may go)
        rc = values_batch_async_impl(g->ws[i], m, dptr.data(), b.nbytes.data(), b.run_base.data(), b.run_len.data(), len,
                                     canonical, g->shard[i].d_pos, b.offs.data(), b.d_vals, want_u128 != 0);
        sum += count;
    }
    // every entry that may have a launch in flight is waited for, also when a later one failed
    for (uint64_t i = 0; i < N; ++i) {
        if (g->batch[i].seqs.empty()) continue;
        hipError_t e = set_device(g->ws[i]->device);
        if (e == hipSuccess) e = hipStreamSynchronize(g->ws[i]->stream);
        if (e != hipSuccess && rc == MM_OK) rc = hip_fail(e, "values_batch sync");
    }
    if (rc) return rc;
    if (total) *total = sum;
    g->batch_vals_words = (int)words;
    return MM_OK;
}

int mm_device_group_batch_values(const mm_device_group_t *g, uint64_t seq, int *entry, uint64_t **d_values, uint64_t *count) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!g || !g->batch_ran || !g->batch_vals_words || seq >= g->seq_entry.size()) return MM_ERR_NULL;
    const int e = g->seq_entry[seq];
    const mm_device_group::BatchEntry &b = g->batch[(size_t)e];
    const uint64_t j = g->seq_slot[seq];
    if (entry) *entry = e;
    if (d_values) *d_values = b.d_vals ? b.d_vals + (uint64_t)g->batch_vals_words * b.offs[j] : nullptr;
    if (count) *count = b.offs[j + 1] - b.offs[j];
    return MM_OK;
}

int mm_device_group_gather_batch(mm_device_group_t *g, int root, uint32_t *d_dst_pos, uint32_t *d_dst_sk,
                                 uint64_t capacity, uint64_t *out_offsets) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (!g || !g->batch_ran || root < 0 || (size_t)root >= g->ws.size() || !out_offsets) return MM_ERR_NULL;
    const uint64_t n_seqs = g->seq_entry.size();
    out_offsets[0] = 0;
    for (uint64_t s = 0; s < n_seqs; ++s) {
        const mm_device_group::BatchEntry &b = g->batch[(size_t)g->seq_entry[s]];
        out_offsets[s + 1] = out_offsets[s] + (b.offs[g->seq_slot[s] + 1] - b.offs[g->seq_slot[s]]);
    }
    if (out_offsets[n_seqs] > capacity) return MM_ERR_CAPACITY;
    if (out_offsets[n_seqs] && !d_dst_pos) return MM_ERR_NULL;
    const int root_dev = g->ws[(size_t)root]->device;
    for (uint64_t s = 0; s < n_seqs; ++s) {
        const int e = g->seq_entry[s];
        const mm_device_group::BatchEntry &b = g->batch[(size_t)e];
        const mm_device_group::Shard &sh = g->shard[(size_t)e];
        mm_workspace *ws = g->ws[(size_t)e];
        const uint64_t j = g->seq_slot[s], c = b.offs[j + 1] - b.offs[j];
        if (!c) continue;
        if (d_dst_sk && !sh.has_sk) return MM_ERR_BAD_MODE;
        // every copy on its SOURCE entry's stream: the entries' copies run side by side
        MM_HIP(set_device(ws->device));
        MM_HIP(hipMemcpyPeerAsync(d_dst_pos + out_offsets[s], root_dev, sh.d_pos + b.offs[j], ws->device, c * sizeof(uint32_t), ws->stream));
        if (d_dst_sk)
            MM_HIP(hipMemcpyPeerAsync(d_dst_sk + out_offsets[s], root_dev, sh.d_sk + b.offs[j], ws->device, c * sizeof(uint32_t), ws->stream));
    }
    for (size_t i = 0; i < g->ws.size(); ++i) {
        MM_HIP(set_device(g->ws[i]->device));
        MM_HIP(hipStreamSynchronize(g->ws[i]->stream));
    }
    return MM_OK;
}

int mm_run_batch_sharded_host(const mm_plan_t *plan, mm_device_group_t *g, uint64_t n_seqs,
                              const uint8_t *const *packed, const uint64_t *base_offsets, const uint64_t *n_bases,
                              uint32_t *out_pos, uint32_t *out_sk, uint64_t capacity, uint64_t *out_offsets) {
    ApiScope api_scope;  // (restores the calling thread's current device on return)
    if (const int bad = dna_plan_only(plan)) return bad;
    if (!plan || !g || g->ws.empty() || !out_offsets) return MM_ERR_NULL;
    if (n_seqs && (!packed || !n_bases)) return MM_ERR_NULL;
    if (out_sk && plan->mode != MM_MINIMIZERS) return MM_ERR_BAD_MODE;
    const uint64_t N = g->ws.size();
    for (uint64_t s = 0; s <= n_seqs; ++s) out_offsets[s] = 0;
    if (n_seqs == 0) return MM_OK;
    // greedy placement, longest sequence first onto the least loaded shard (sharding.assign_contigs)
    std::vector<uint64_t> order(n_seqs);
    for (uint64_t s = 0; s < n_seqs; ++s) order[s] = s;
    std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return n_bases[a] > n_bases[b]; });
    std::vector<std::vector<uint64_t>> mine(N);
    std::vector<uint64_t> load(N, 0);
    for (uint64_t s : order) {
        uint64_t best = 0;
        for (uint64_t i = 1; i < N; ++i)
            if (load[i] < load[best]) best = i;
        mine[best].push_back(s);
        load[best] += n_bases[s];
    }
    for (uint64_t i = 0; i < N; ++i) std::sort(mine[i].begin(), mine[i].end());
    std::vector<ShardResult> res(N);
    std::vector<std::vector<uint64_t>> local_offs(N);  // per shard: offsets of its sequences in its staging buffer
    auto phase1 = [&](uint64_t i) {
        ShardResult &r = res[i];
        mm_workspace *ws = g->ws[i];
        const std::vector<uint64_t> &my = mine[i];
        if (my.empty()) return;
        auto fail = [&](int rc) {
            r.rc = rc;
            r.err = g_last_error;
        };
        if (set_device(ws->device) != hipSuccess) return fail(MM_ERR_HIP);
        // the shard's sequences back to back in one device buffer, each at a 16-byte boundary
        std::vector<uint64_t> at(my.size()), nbytes(my.size());
        uint64_t total = 0, windows = 0;
        const uint64_t l = (uint64_t)plan->k + plan->w - 1;
        for (size_t j = 0; j < my.size(); ++j) {
            const uint64_t s = my[j];
            nbytes[j] = ((base_offsets ? base_offsets[s] : 0) + n_bases[s] + 3) / 4;
            at[j] = total;
            total += (nbytes[j] + 16 + 15) & ~15ull;
            windows += n_bases[s] >= l ? n_bases[s] - l + 1 : 0;
        }
        int rc = grow_bytes(ws->d_in, ws->d_in_bytes, total + 16);
        if (rc) return fail(rc);
        uint8_t *const din = static_cast<uint8_t *>(ws->d_in);
        std::vector<const void *> dptr(my.size());
        std::vector<uint64_t> dbytes(my.size()), offs(my.size()), lens(my.size());
        for (size_t j = 0; j < my.size(); ++j) {
            const uint64_t s = my[j];
            if (nbytes[j]) {
                if (!packed[s]) return fail(MM_ERR_NULL);
                if (hipMemcpyAsync(din + at[j], packed[s], nbytes[j], hipMemcpyHostToDevice, ws->stream) != hipSuccess)
                    return fail(MM_ERR_HIP);
            }
            dptr[j] = din + at[j];
            dbytes[j] = nbytes[j] + 16;
            offs[j] = base_offsets ? base_offsets[s] : 0;
            lens[j] = n_bases[s];
        }
        const uint64_t cap = out_pos ? (windows < capacity ? windows : capacity) : 0;
        rc = grow(ws->d_out, ws->d_out_elems, cap ? cap : 1, sizeof(uint32_t));
        if (rc == MM_OK && out_sk) rc = grow(ws->d_sk, ws->d_sk_elems, cap ? cap : 1, sizeof(uint32_t));
        if (rc) return fail(rc);
        local_offs[i].assign(my.size() + 1, 0);
        rc = mm_run_batch_device(plan, ws, my.size(), dptr.data(), dbytes.data(), offs.data(), lens.data(),
                                 cap ? ws->d_out : nullptr, (out_sk && cap) ? ws->d_sk : nullptr, cap,
                                 local_offs[i].data());
        r.count = local_offs[i][my.size()];
        if (rc && rc != MM_ERR_CAPACITY) return fail(rc);
        r.rc = rc;
    };
    {
        std::vector<std::thread> th;
        for (uint64_t i = 1; i < N; ++i) th.emplace_back(phase1, i);
        phase1(0);
        for (std::thread &t : th) t.join();
    }
    bool over = false;
    for (uint64_t i = 0; i < N; ++i) {
        if (res[i].rc == MM_ERR_CAPACITY) over = true;
        else if (res[i].rc) {
            g_last_error = res[i].err;
            return res[i].rc;
        }
    }
    // counts per sequence (input order) -> offsets in the caller's buffer
    std::vector<uint64_t> cnt(n_seqs, 0);
    for (uint64_t i = 0; i < N; ++i)
        for (size_t j = 0; j < mine[i].size(); ++j) cnt[mine[i][j]] = local_offs[i][j + 1] - local_offs[i][j];
    for (uint64_t s = 0; s < n_seqs; ++s) out_offsets[s + 1] = out_offsets[s] + cnt[s];
    if (over || (out_pos && out_offsets[n_seqs] > capacity)) return MM_ERR_CAPACITY;
    if (!out_pos) return MM_OK;
    auto phase2 = [&](uint64_t i) {
        mm_workspace *ws = g->ws[i];
        if (mine[i].empty()) return;
        bool bad = set_device(ws->device) != hipSuccess;
        // (runs of sequences that are neighbours in the input are neighbours in both buffers: one copy per run)
        for (size_t j = 0; j < mine[i].size() && !bad;) {
            size_t e = j + 1;
            while (e < mine[i].size() && mine[i][e] == mine[i][e - 1] + 1) ++e;
            bad = copy_shard_out(ws, local_offs[i][j], local_offs[i][e] - local_offs[i][j], out_pos, out_sk,
                                 out_offsets[mine[i][j]]) != MM_OK;
            j = e;
        }
        if (!bad) bad = hipStreamSynchronize(ws->stream) != hipSuccess;
        if (bad) {
            res[i].rc = MM_ERR_HIP;
            res[i].err = g_last_error;
        }
    };
    {
        std::vector<std::thread> th;
        for (uint64_t i = 1; i < N; ++i) th.emplace_back(phase2, i);
        phase2(0);
        for (std::thread &t : th) t.join();
    }
    for (uint64_t i = 0; i < N; ++i)
        if (res[i].rc) {
            g_last_error = res[i].err;
            return res[i].rc;
        }
    return MM_OK;
}

}  // extern "C"

// What the FASTA / FASTQ stream (mm_fastx_stream.hip) asks of the file that owns plans and workspaces (mm_fastx_stream.h).
#include "mm_fastx_stream.h"
namespace mm {
ApiPlanInfo api_plan_info(const mm_plan_t *plan) {
    ApiPlanInfo i;
    i.k = plan->k;
    i.w = plan->w;
    i.mode = plan->mode;
    i.canonical_windows = plan->canonical_windows;
    i.canonical_hasher = plan->text ? (int)plan->tt.canonical : (int)plan->hasher.canonical;
    i.text = plan->text ? 1 : 0;
    return i;
}
int api_reads_counts_refusal(const mm_plan_t *plan, uint64_t max_bases, uint64_t max_records, int want_sk, int want_amb) {
    // (the check reads no pointer: any non-null value stands for the buffers, and for a workspace with no knob set)
    static uint64_t some = 0;
    const AmbArgs amb{&some, ~0ull >> 3, 0};
    const int r = packed_reads_counts_check(
        plan, nullptr, {.d_packed = &some, .packed_bytes = ~0ull >> 2, .max_bases = max_bases, .max_records = max_records,
                        .d_read_starts = &some, .d_counts = &some, .d_out_sk = want_sk ? reinterpret_cast<uint32_t *>(&some) : nullptr,
                        .d_out_offsets = &some, .amb = want_amb ? &amb : nullptr});
    return r == MM_ERR_NULL && plan ? (int)MM_OK : r;  // (MM_ERR_NULL with a plan: the missing workspace, refused last)
}
int api_text_counts_refusal(const mm_plan_t *plan, uint64_t max_chars, uint64_t max_records, int want_sk) {
    // (the check reads no pointer: any non-null value stands for the buffers)
    static uint64_t some = 0;
    return text_batch_counts_check(plan, {.d_text = &some, .text_bytes = ~0ull, .max_chars = max_chars, .max_records = max_records,
                                          .d_starts = &some, .d_counts = &some,
                                          .d_out_sk = want_sk ? reinterpret_cast<uint32_t *>(&some) : nullptr,
                                          .d_out_offsets = &some});
}
int api_one_min_text_plan_counts(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_text, uint64_t text_bytes,
                                 uint64_t max_chars, uint64_t max_records, const uint64_t *d_starts, const uint64_t *d_counts,
                                 uint32_t *d_out_pos) {
    if (!plan || !plan->text) return MM_ERR_BAD_MODE;
    const int r = one_min_counts_check(ws, plan, plan->k, d_text, text_bytes, 0, max_chars, max_records, d_starts, d_counts,
                                       d_out_pos);
    if (r || max_records == 0) return r;
    return one_min_text_counts_queue(ws, plan->tt, plan->k, d_text, max_chars, max_records, d_starts, d_counts, d_out_pos);
}
int api_one_min_reads_plan_counts(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed, uint64_t packed_bytes,
                                  const void *d_amb, uint64_t amb_bytes, uint64_t max_bases, uint64_t max_records,
                                  const uint64_t *d_read_starts, const uint64_t *d_counts, uint32_t *d_out_pos) {
    if (!plan || plan->text) return MM_ERR_BAD_MODE;
    const OneMinAmbBits amb{d_amb, amb_bytes, 0};
    return one_min_reads_counts(ws, &plan->hasher, plan->k, d_packed, packed_bytes, 0, max_bases, max_records, d_read_starts,
                                d_counts, d_out_pos, d_amb ? &amb : nullptr);
}
hipStream_t api_workspace_stream(mm_workspace_t *ws) { return ws->stream; }
void api_set_last_error(const char *text) { g_last_error = text; }
// (mm_bgzf.h)
uint32_t *api_workspace_error(mm_workspace_t *ws) { return error_word(ws); }
int api_workspace_device(mm_workspace_t *ws) { return ws->device; }
void api_workspace_mark_async(mm_workspace_t *ws) { ws->async_unchecked = true; }
}  // namespace mm
