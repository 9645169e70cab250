// mm_fastx_stream.hip - FASTA / FASTQ files of ANY size through the device in chunks (mm_fastx_stream_*, host code).
//
// The reference's loader reads a file of any size record by record on the CPU (needletail::parse_fastx_file,
// bench/src/lib.rs:51-82) and runs the builder per record (src/lib.rs:378); beyond that it has no counterpart.  Here the
// caller feeds bytes, the stream cuts them into chunks of chunk_bytes, and every chunk goes through the calls that exist
// for a whole file - packer, counts run, values - on a slot of its own:
//   slot = a workspace (its own stream), a page-locked staging buffer for chunk_bytes of text, device buffers for a text
//          of 2 * chunk_bytes (the carry area in front of the new bytes) and the outputs, page-locked landing buffers.
//   launch(chunk i + 1): upload of the new bytes - queued BEFORE the host looks at chunk i's cut; wait for the 32 bytes
//          {B', R', cut, overflow} of chunk i (they arrive behind its packer and trim step, ahead of its run); device copy
//          of chunk i's tail text[cut, n) directly in front of the new bytes; packer; trim (mm_fastx_cut.hip); the counts
//          run; values; the run's count to the host.
//   collect(chunk): once the count is on the host, the downloads of exactly the filled parts are queued; the batch is
//          complete when they are done.  feed() and next() both move chunks along, neither waits unless it must.
// A tail always lies inside its chunk's NEW bytes (a chunk whose cut is 0 is an error), so it is at most chunk_bytes long.
//
// MM_FASTX_LONG_RECORDS (FASTA text): a chunk that is one record from its first byte on and has no cut is a PIECE of an open
// record (the split rule of mm_fastx_cut.h).  The chunk behind it starts with ">\n" and the piece's last l - 1 sequence
// bytes text[T, n) in place of a tail, so packer, run and values work on it unchanged; behind the values the seam
// epilogue's kernel adds first_base to record 0's positions (queue_run), and mm_fastx_stream_next, which hands the batches
// out in text order, drops a minimizer piece's first position when the record emitted it last (the reference's rule for
// joining lanes, src/collect.rs:265-271).  Nothing crosses from slot to slot on the device, so a repeated run repeats
// nothing but its own slot's work.
//
// BYTE TEXT (mm_fastx_text_stream_create: a text plan, protein FASTA): the same slots and steps; the loader is
// mm_fasta_text_device_async, whose sequence bytes go where the packed bases go (d_packed: 2 * chunk_bytes bytes), whose
// starts go into d_rec_base and whose counts have the packers' layout, so the trim step is used as it is; the run and the
// values are the text batch counts calls, and MM_FASTX_TEXT_ONE_MINIMIZER adds the one-minimizer counts call behind them.
//
// MM_FASTX_ONE_MINIMIZER (the DNA stream): behind the run and the values, on the slot's stream, the packed one-minimizer
// counts call - with MM_FASTX_SKIP_AMBIGUOUS its skip-ambiguous form over the slot's d_amb - writes one word per record
// into d_one; the delivered records' words are downloaded with the batch (mm_fastx_stream_one_minimizer).  Still one host
// wait per chunk.  Refused with MM_FASTX_LONG_RECORDS: a split record's minimizer is not joined across its pieces.
//
// BGZF INPUT (mm_fastx_stream_feed_bgzf): only how a slot's new bytes arrive changes.  Whole BGZF blocks are gathered into a
// page-locked compressed staging buffer of the slot with a block table (payload offset, sizes, where the text goes); at the
// launch the staging buffer and the table are uploaded in place of the text and the inflate kernel (mm_bgzf.hip, one
// wavefront per block) writes d_text + A + out_off on the slot's stream, the packer behind it.  A slot's new bytes are
// host bytes (h_text: what mm_fastx_stream_feed brought, and the stream's first blocks, inflated on the host so that
// MM_FASTX_AUTO and the blank bytes in front of a text go through the one rule of feed) followed by device-inflated
// blocks; a chunk carries UP TO chunk_bytes new bytes (the next block would not fit), which launch() and the trim step
// never took for exactly chunk_bytes.  The workspace's sticky error word comes to the host with the cut, so a block
// that did not inflate fails the stream with MM_ERR_FORMAT before anything is made of its text.  With MM_FASTX_BGZF_CRC the
// trailers' CRC32s go up with the table, the inflate writes a status array and the verify kernel (mm_crc32.hip, one workgroup
// per block) runs behind it, in front of the copy of the sticky word: a mismatch fails the stream the same way, "CRC32" in
// its text.  The host-inflated blocks are checked on the host.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "mm_bgzf.h"
#include "mm_crc32.h"
#include "mm_fastx_cut.h"
#include "mm_fastx_stream.h"
#include "mm_inflate.h"

namespace {

enum SlotState { kFree = 0, kFilling, kRunning, kDownloading, kDelivered };

struct Slot {
    mm_workspace_t *ws = nullptr;
    hipStream_t stream = nullptr;
    // device
    uint8_t *d_text = nullptr;  // [A + chunk_bytes + 64]: carry area (A bytes), then the new bytes
    uint8_t *d_packed = nullptr, *d_amb = nullptr;
    uint64_t *d_rec_base = nullptr, *d_rec_pos = nullptr, *d_offsets = nullptr;
    unsigned long long *d_meta = nullptr;  // [0..1] bases, records  [2..6] cut, overflow, T, open, overlap  [7] positions  [8] newlines
    uint32_t *d_pos = nullptr, *d_sk = nullptr;
    uint64_t *d_values = nullptr;
    uint32_t *d_one = nullptr;  // MM_FASTX_TEXT_ONE_MINIMIZER / MM_FASTX_ONE_MINIMIZER: one word per record
    // page-locked host
    uint8_t *h_text = nullptr;
    unsigned long long *h_meta = nullptr;  // words 0..7 of d_meta; bytes 120..121: the synthetic header line ">\n"
    uint64_t *h_rec_pos = nullptr, *h_rec_base = nullptr, *h_offsets = nullptr, *h_values = nullptr;
    uint32_t *h_pos = nullptr, *h_sk = nullptr;
    uint32_t *h_one = nullptr;  // the one-minimizer words ...
    uint8_t *h_seq = nullptr;   // ... and, byte text, the records' bytes (MM_FASTX_TEXT_SEQ)
    // BGZF input (allocated by the first mm_fastx_stream_feed_bgzf): compressed payloads back to back and their table,
    // page-locked, and their device twins; n_blk_bytes of the slot's n_new bytes come from the n_blk blocks, behind the
    // n_new - n_blk_bytes bytes of h_text
    uint8_t *h_comp = nullptr, *d_comp = nullptr;
    mm_bgzf_block_t *h_blocks = nullptr, *d_blocks = nullptr;
    uint64_t n_comp = 0, n_blk = 0, n_blk_bytes = 0;
    // MM_FASTX_BGZF_CRC: the blocks' trailer CRC32s beside the table (table_max words each), and the status array that the
    // inflate writes and the verify kernel reads
    uint32_t *h_crc = nullptr, *d_crc = nullptr, *d_status = nullptr;
    hipEvent_t ev_cut = nullptr, ev_run = nullptr, ev_done = nullptr, ev_tail = nullptr;
    bool tail_pending = false;  // the chunk behind this slot's copies its tail out of d_text: ev_tail says when it has
    // the chunk in the slot
    SlotState state = kFree;
    uint64_t n_new = 0, n_text = 0, text_off = 0, abs_begin = 0, report_begin = 0;
    int last = 0, retries = 0;
    // MM_FASTX_LONG_RECORDS: record 0 continues the open record of the chunk before
    bool continues = false;
    uint64_t first_base = 0, first_overlap = 0, rec0_pos = 0;  // rec0_pos: the absolute offset of the record's real '>'
};

struct DeviceGuard {  // every entry restores the caller's current device
    int saved = -1;
    DeviceGuard() {
        if (hipGetDevice(&saved) != hipSuccess) {
            (void)hipGetLastError();
            saved = -1;
        }
    }
    ~DeviceGuard() {
        if (saved >= 0) (void)hipSetDevice(saved);
    }
};

}  // namespace

struct mm_fastx_stream {
    const mm_plan_t *plan = nullptr;
    mm::ApiPlanInfo info{};
    mm_fastx_stream_config_t cfg{};
    uint32_t value_len = 0;
    uint64_t C = 0, max_records = 0, max_positions = 0, packed_cap = 0, amb_cap = 0;
    uint64_t A = 0;  // the carry area in front of the new bytes: C, with MM_FASTX_LONG_RECORDS C + 16 (2 bytes of it are used)
    // MM_FASTX_LONG_RECORDS, in the order of delivery: the last position the open record has emitted
    bool have_last = false;
    uint32_t last_emitted = 0;
    mm_fastx_pieces_t pieces{};  // of the batch handed out last
    // a stream of mm_fastx_text_stream_create: byte text, d_packed holds the sequence bytes (packed_cap of them)
    bool text = false;
    int values_encoding = 0;
    mm_fastx_text_extras_t extras{};  // of the batch handed out last
    int n_slots = 0;
    Slot slots[8];
    int fill = 0;      // the slot that takes the bytes fed next
    int oldest = 0;    // the oldest launched slot that next() has not delivered yet
    int in_flight = 0; // launched, not delivered
    int prev = -1;     // the slot of the chunk launched last (its tail goes in front of the next one)
    int delivered = -1;
    int format = 0;    // MM_FASTX_FASTA / MM_FASTX_FASTQ once it is known
    std::string line_blanks;  // MM_FASTX_AUTO, before the first non-blank byte: the blank bytes of the line it stands in
    uint64_t skipped = 0;     // blank bytes in front of the text that were not handed to a packer
    bool any_launched = false, finished = false, final_done = false;
    // BGZF input: feed_bgzf was called (mm_fastx_stream_feed is refused from then on); its last call ended inside a block
    bool bgzf = false, bgzf_partial = false;
    uint64_t comp_cap = 0, table_max = 0;
    std::vector<uint8_t> bgzf_first;  // the text of a block inflated on the host
    int failed = 0;
    std::string fail_text;
};

namespace {

int fail(mm_fastx_stream *s, int code, const std::string &text) {
    s->failed = code;
    s->fail_text = text;
    mm::api_set_last_error(s->fail_text.c_str());
    return code;
}
int fail_hip(mm_fastx_stream *s, hipError_t e, const char *what) {
    return fail(s, MM_ERR_HIP, std::string("mm_fastx_stream: ") + what + ": " + hipGetErrorString(e));
}
// (a failed call of the library: its own text stands in mm_last_error())
int fail_call(mm_fastx_stream *s, int code) { return fail(s, code, std::string("mm_fastx_stream: ") + mm_last_error()); }
int again(mm_fastx_stream *s) {
    mm::api_set_last_error(s->fail_text.c_str());
    return s->failed;
}
#define FX_HIP(call)                                         \
    do {                                                     \
        hipError_t e_ = (call);                              \
        if (e_ != hipSuccess) return fail_hip(s, e_, #call); \
    } while (0)

// a slot whose chunk is gone: no new bytes of either kind
void clear_new(Slot &sl) {
    sl.n_new = sl.n_comp = sl.n_blk = sl.n_blk_bytes = 0;
    sl.h_meta[9] = 0;
}
// BGZF input: the chunk's inflate - or, with MM_FASTX_BGZF_CRC, the verify kernel behind it - raised its error (read behind
// ev_cut, before anything is made of the chunk's text)
bool bgzf_failed(const Slot &sl) {
    return sl.n_blk && ((uint32_t)sl.h_meta[9] == mm::kErrBgzfBlock || (uint32_t)sl.h_meta[9] == mm::kErrBgzfCrc);
}
int fail_bgzf(mm_fastx_stream *s) {
    return fail(s, MM_ERR_FORMAT, "mm_fastx_stream: a BGZF block did not inflate (not deflate, or not ISIZE bytes of it)");
}
int fail_crc(mm_fastx_stream *s) {
    return fail(s, MM_ERR_FORMAT, "mm_fastx_stream: CRC32 mismatch: a BGZF block's text does not have the CRC32 of its gzip trailer "
                                  "(the file is corrupt)");
}
// (the sticky word keeps the larger code: a chunk with both kinds of failure reports the mismatch)
int fail_bgzf(mm_fastx_stream *s, const Slot &sl) { return (uint32_t)sl.h_meta[9] == mm::kErrBgzfCrc ? fail_crc(s) : fail_bgzf(s); }

bool is_blank(uint8_t c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n'; }
bool can_fill(const Slot &sl) { return sl.state == kFree || sl.state == kFilling; }
// the split rule is in force: the flag, on FASTA text (a FASTQ stream behaves as without it)
bool long_fasta(const mm_fastx_stream *s) { return (s->cfg.flags & MM_FASTX_LONG_RECORDS) && s->format == MM_FASTX_FASTA; }

// steps 5-7 of a launched slot: the counts run, the values, the run's count to the host (queued again after a look-back
// time-out: the packed records and the trimmed counts are still where the run reads them)
int queue_run(mm_fastx_stream *s, Slot &sl) {
    const uint32_t flags = s->cfg.flags;
    uint64_t *const d_counts = reinterpret_cast<uint64_t *>(sl.d_meta), *const d_count = reinterpret_cast<uint64_t *>(sl.d_meta + 7);
    const uint64_t max_bases = sl.n_text - (sl.continues ? 2 : 0);  // (the synthetic header line holds no base)
    int r;
    if (s->text) {
        // (max_chars = the chunk's text length: it bounds the characters the loader can have written)
        r = mm_run_text_batch_counts_device_async(s->plan, sl.ws, sl.d_packed, s->packed_cap, sl.n_text, s->max_records,
                                                  sl.d_rec_base, d_counts, sl.d_pos, sl.d_sk, s->max_positions, sl.d_offsets, d_count);
        if (r) return fail_call(s, r);
        if (sl.d_values && s->max_records) {
            r = (flags & MM_FASTX_VALUES_U128 ? mm_values_u128_text_batch_counts_device_async
                                              : mm_values_u64_text_batch_counts_device_async)(
                sl.ws, sl.d_packed, s->packed_cap, sl.n_text, s->max_records, sl.d_rec_base, d_counts, s->values_encoding,
                s->value_len, s->info.canonical_hasher, sl.d_pos, sl.d_offsets, s->max_positions, sl.d_values);
            if (r) return fail_call(s, r);
        }
        if (sl.d_one && s->max_records) {
            r = mm::api_one_min_text_plan_counts(s->plan, sl.ws, sl.d_packed, s->packed_cap, sl.n_text, s->max_records,
                                                 sl.d_rec_base, d_counts, sl.d_one);
            if (r) return fail_call(s, r);
        }
        FX_HIP(hipSetDevice(s->cfg.device));
        FX_HIP(hipMemcpyAsync(sl.h_meta + 7, sl.d_meta + 7, sizeof(unsigned long long), hipMemcpyDeviceToHost, sl.stream));
        FX_HIP(hipEventRecord(sl.ev_run, sl.stream));
        return MM_OK;
    }
    if (flags & MM_FASTX_SKIP_AMBIGUOUS)
        r = mm_run_packed_reads_skip_ambiguous_counts_device_async(s->plan, sl.ws, sl.d_packed, s->packed_cap, 0, sl.d_amb, s->amb_cap, 0,
                                                                   max_bases, s->max_records, sl.d_rec_base, d_counts, sl.d_pos,
                                                                   s->max_positions, sl.d_offsets, d_count);
    else
        r = mm_run_packed_reads_counts_device_async(s->plan, sl.ws, sl.d_packed, s->packed_cap, 0, max_bases, s->max_records,
                                                    sl.d_rec_base, d_counts, sl.d_pos, sl.d_sk, s->max_positions, sl.d_offsets, d_count);
    if (r) return fail_call(s, r);
    if (sl.d_values && s->max_records) {
        r = (flags & MM_FASTX_VALUES_U128 ? mm_values_u128_reads_device_async : mm_values_u64_reads_device_async)(
            sl.ws, sl.d_packed, s->packed_cap, 0, s->max_records, sl.d_rec_base, 0, s->value_len, s->info.canonical_windows, sl.d_pos,
            sl.d_offsets, s->max_positions, sl.d_values);
        if (r) return fail_call(s, r);
    }
    // (the trimmed counts: the records the batch delivers; a repeated run queues the call again)
    if (sl.d_one && s->max_records) {
        r = mm::api_one_min_reads_plan_counts(s->plan, sl.ws, sl.d_packed, s->packed_cap,
                                              (flags & MM_FASTX_SKIP_AMBIGUOUS) ? sl.d_amb : nullptr, s->amb_cap, max_bases,
                                              s->max_records, sl.d_rec_base, d_counts, sl.d_one);
        if (r) return fail_call(s, r);
    }
    FX_HIP(hipSetDevice(s->cfg.device));
    // the seam epilogue's device part, behind the values (they read k-mers at piece-local positions): record 0's positions
    // and window indices become record-global.  A repeated run writes the slice anew, so the bias is never added twice.
    if (sl.continues && mm::launch_fastx_bias(sl.d_meta, reinterpret_cast<unsigned long long *>(sl.d_offsets), s->max_records,
                                              s->max_positions, (uint32_t)sl.first_base, sl.d_pos, sl.d_sk, sl.stream))
        return fail_hip(s, hipGetLastError(), "the seam epilogue");
    FX_HIP(hipMemcpyAsync(sl.h_meta + 7, sl.d_meta + 7, sizeof(unsigned long long), hipMemcpyDeviceToHost, sl.stream));
    FX_HIP(hipEventRecord(sl.ev_run, sl.stream));
    return MM_OK;
}

// Launches the chunk in the filling slot (steps 1-7).  `last`: nothing follows.  A last chunk without a byte - no new one,
// no tail - is not launched.
int launch(mm_fastx_stream *s, int last) {
    Slot &sl = s->slots[s->fill];
    FX_HIP(hipSetDevice(s->cfg.device));
    // (this slot's previous chunk: the chunk behind it may still be copying its tail out of d_text)
    if (sl.tail_pending) {
        FX_HIP(hipStreamWaitEvent(sl.stream, sl.ev_tail, 0));
        sl.tail_pending = false;
    }
    const uint64_t n_host = sl.n_new - sl.n_blk_bytes;
    if (n_host) FX_HIP(hipMemcpyAsync(sl.d_text + s->A, sl.h_text, n_host, hipMemcpyHostToDevice, sl.stream));
    if (sl.n_blk) {
        // BGZF blocks: the compressed bytes and their table in place of the text; the blocks' slots lie behind the host bytes
        FX_HIP(hipMemcpyAsync(sl.d_comp, sl.h_comp, sl.n_comp, hipMemcpyHostToDevice, sl.stream));
        FX_HIP(hipMemcpyAsync(sl.d_blocks, sl.h_blocks, sl.n_blk * sizeof(mm_bgzf_block_t), hipMemcpyHostToDevice, sl.stream));
        uint32_t *const err = mm::api_workspace_error(sl.ws);
        mm::api_workspace_mark_async(sl.ws);
        const bool verify = (s->cfg.flags & MM_FASTX_BGZF_CRC) != 0;
        if (verify) FX_HIP(hipMemcpyAsync(sl.d_crc, sl.h_crc, sl.n_blk * sizeof(uint32_t), hipMemcpyHostToDevice, sl.stream));
        // (the inflate writes every block's status word; the verify kernel skips the blocks it has failed)
        if (mm::launch_bgzf_inflate(sl.d_comp, sl.n_comp, sl.d_blocks, sl.n_blk, sl.d_text + s->A, sl.n_new, verify ? sl.d_status : nullptr,
                                    err, sl.stream))
            return fail_hip(s, hipGetLastError(), "the BGZF inflate");
        if (verify && mm::launch_bgzf_crc32(sl.d_text + s->A, sl.n_new, sl.d_blocks, sl.n_blk, sl.d_crc, nullptr, sl.d_status, err, sl.stream))
            return fail_hip(s, hipGetLastError(), "the BGZF CRC32");
        // (the sticky error word, as the inflate and the verify left it: on the host with the cut)
        FX_HIP(hipMemcpyAsync(sl.h_meta + 9, err + 2, sizeof(uint32_t), hipMemcpyDeviceToHost, sl.stream));
    }
    uint64_t tail = 0;
    sl.continues = false;
    sl.first_base = sl.first_overlap = sl.rec0_pos = 0;
    if (s->prev >= 0) FX_HIP(hipEventSynchronize(s->slots[s->prev].ev_cut));
    if (s->prev >= 0 && bgzf_failed(s->slots[s->prev])) return fail_bgzf(s, s->slots[s->prev]);
    if (s->prev >= 0 && long_fasta(s) && s->slots[s->prev].h_meta[5] && !s->slots[s->prev].h_meta[3]) {
        // the chunk before is a piece of an open record: ">\n", its last l - 1 sequence bytes text[T, n), the new bytes
        Slot &p = s->slots[s->prev];
        const uint64_t T = p.h_meta[4], overlap = p.h_meta[6], bases = p.h_meta[0];
        if (T > p.n_text || p.h_meta[2] != p.n_text || overlap > bases)
            return fail(s, MM_ERR_HIP, "mm_fastx_stream: the trim step left counts beyond their bounds");
        if (bases <= p.first_overlap)
            return fail(s, MM_ERR_CAPACITY, "mm_fastx_stream: a piece of " + std::to_string(p.n_text) +
                                                " bytes brings no new base of its record (cannot advance)");
        if (p.first_base + bases >= (1ull << 32))
            return fail(s, MM_ERR_LEN_TOO_LARGE, "mm_fastx_stream: a record of 2^32 bases or more");
        tail = p.n_text - T;
        if (tail > s->C)  // (with the header line a packer sees 2 * chunk_bytes + 2 bytes at most, 2 * chunk_bytes bases)
            return fail(s, MM_ERR_CAPACITY, "mm_fastx_stream: the overlap of a split record is longer than chunk_bytes");
        uint8_t *const dst = sl.d_text + s->A - tail - 2;
        FX_HIP(hipMemcpyAsync(dst, reinterpret_cast<const uint8_t *>(sl.h_meta) + 120, 2, hipMemcpyHostToDevice, sl.stream));
        if (tail) FX_HIP(hipMemcpyAsync(dst + 2, p.d_text + p.text_off + T, tail, hipMemcpyDeviceToDevice, sl.stream));
        FX_HIP(hipEventRecord(p.ev_tail, sl.stream));
        p.tail_pending = true;
        sl.continues = true;
        sl.first_base = p.first_base + bases - overlap;
        sl.first_overlap = overlap;
        sl.rec0_pos = p.continues ? p.rec0_pos : p.abs_begin;  // (an open chunk's record starts at its first byte)
        sl.abs_begin = p.abs_begin + T - 2;  // (the header line has two bytes at least, so T >= 2)
        sl.report_begin = p.abs_begin + p.n_text;
        tail += 2;
    } else if (s->prev >= 0) {
        Slot &p = s->slots[s->prev];
        const uint64_t cut = p.h_meta[2];
        // (a chunk that cannot be cut: its own collect step names the reason; nothing can follow it)
        if (p.h_meta[3] || cut == 0 || cut > p.n_text) {
            if (p.h_meta[3])
                return fail(s, MM_ERR_CAPACITY, "mm_fastx_stream: more than max_records = " + std::to_string(s->max_records) +
                                                    " records in a chunk: " + std::to_string(p.h_meta[1]) + " needed");
            return fail(s, MM_ERR_CAPACITY, "mm_fastx_stream: a record longer than chunk_bytes = " + std::to_string(s->C) +
                                                " (no cut in a chunk of " + std::to_string(p.n_text) + " bytes)");
        }
        tail = p.n_text - cut;
        if (tail > s->C) return fail(s, MM_ERR_CAPACITY, "mm_fastx_stream: a tail longer than chunk_bytes");
        if (tail) {
            FX_HIP(hipMemcpyAsync(sl.d_text + s->A - tail, p.d_text + p.text_off + cut, tail, hipMemcpyDeviceToDevice, sl.stream));
            FX_HIP(hipEventRecord(p.ev_tail, sl.stream));
            p.tail_pending = true;
        }
        sl.abs_begin = p.abs_begin + cut;
        sl.report_begin = sl.abs_begin;
    } else {
        sl.abs_begin = s->cfg.first_byte + s->skipped;
        sl.report_begin = s->cfg.first_byte;
    }
    sl.n_text = tail + sl.n_new;
    sl.text_off = s->A - tail;
    sl.last = last;
    sl.retries = 0;
    if (sl.n_text == 0) {  // (only a last chunk comes here without a byte)
        sl.state = kFree;
        clear_new(sl);
        return MM_OK;
    }
    const uint8_t *text = sl.d_text + sl.text_off;
    uint64_t *const d_counts = reinterpret_cast<uint64_t *>(sl.d_meta);
    int r;
    if (s->text)
        r = mm_fasta_text_device_async(sl.ws, text, sl.n_text, sl.d_packed, s->packed_cap, sl.d_rec_base, sl.d_rec_pos,
                                       s->max_records, d_counts);
    else if (s->cfg.flags & MM_FASTX_SKIP_AMBIGUOUS)
        r = (s->format == MM_FASTX_FASTQ ? mm_fastq_pack_n_device_async : mm_fasta_pack_n_device_async)(
            sl.ws, text, sl.n_text, sl.d_packed, s->packed_cap, sl.d_amb, s->amb_cap, sl.d_rec_base, sl.d_rec_pos, s->max_records, d_counts);
    else
        r = (s->format == MM_FASTX_FASTQ ? mm_fastq_pack_device_async : mm_fasta_pack_device_async)(
            sl.ws, text, sl.n_text, sl.d_packed, s->packed_cap, sl.d_rec_base, sl.d_rec_pos, s->max_records, d_counts);
    if (r) return fail_call(s, r);
    FX_HIP(hipSetDevice(s->cfg.device));
    if (mm::launch_fastx_trim(text, sl.n_text, s->format, last, long_fasta(s) ? 1 : 0, s->info.k + s->info.w - 1,
                              reinterpret_cast<unsigned long long *>(sl.d_rec_base), reinterpret_cast<unsigned long long *>(sl.d_rec_pos),
                              s->max_records, sl.d_meta, sl.d_meta + 2, sl.d_meta + 8, sl.stream))
        return fail_hip(s, hipGetLastError(), "the trim step");
    FX_HIP(hipMemcpyAsync(sl.h_meta, sl.d_meta, 7 * sizeof(unsigned long long), hipMemcpyDeviceToHost, sl.stream));
    FX_HIP(hipEventRecord(sl.ev_cut, sl.stream));
    r = queue_run(s, sl);
    if (r) return r;
    sl.state = kRunning;
    s->prev = s->fill;
    s->any_launched = true;
    if (s->in_flight == 0) s->oldest = s->fill;
    ++s->in_flight;
    s->fill = (s->fill + 1) % s->n_slots;
    return MM_OK;
}

// A running slot whose count has arrived (or, with `block`, once it has): judge the run, queue the downloads.
int collect(mm_fastx_stream *s, Slot &sl, bool block) {
    while (sl.state == kRunning) {
        if (!block) {
            const hipError_t q = hipEventQuery(sl.ev_run);
            if (q == hipErrorNotReady) {
                (void)hipGetLastError();  // (not an error: the launchers ask for the last one)
                return MM_OK;
            }
            if (q != hipSuccess) return fail_hip(s, q, "hipEventQuery");
        }
        FX_HIP(hipEventSynchronize(sl.ev_run));
        if (bgzf_failed(sl)) return fail_bgzf(s, sl);
        const int r = mm_workspace_check(sl.ws);
        if (r == MM_ERR_ORDER && sl.retries < 2) {
            // a look-back timed out: this chunk's run again (the workspace takes its tile ids from a ticket from now on)
            ++sl.retries;
            const int q = queue_run(s, sl);
            if (q) return q;
            continue;
        }
        const uint64_t n_bases = sl.h_meta[0], n_records = sl.h_meta[1], cut = sl.h_meta[2], n_pos = sl.h_meta[7];
        if (sl.h_meta[3])
            return fail(s, MM_ERR_CAPACITY, "mm_fastx_stream: more than max_records = " + std::to_string(s->max_records) +
                                                " records in a chunk: " + std::to_string(n_records) + " needed");
        if (r) return fail_call(s, r);
        if (!sl.last && cut == 0)
            return fail(s, MM_ERR_CAPACITY, "mm_fastx_stream: a record longer than chunk_bytes = " + std::to_string(s->C) +
                                                " (no cut in a chunk of " + std::to_string(sl.n_text) + " bytes)");
        if (n_pos > s->max_positions)
            return fail(s, MM_ERR_CAPACITY, "mm_fastx_stream: more than max_positions = " + std::to_string(s->max_positions) +
                                                " positions in a chunk: " + std::to_string(n_pos) + " needed");
        if (n_records > s->max_records || n_bases > sl.n_text || cut > sl.n_text)
            return fail(s, MM_ERR_HIP, "mm_fastx_stream: the trim step left counts beyond their bounds");
        FX_HIP(hipSetDevice(s->cfg.device));
        if (sl.d_one && n_records) FX_HIP(hipMemcpyAsync(sl.h_one, sl.d_one, n_records * 4, hipMemcpyDeviceToHost, sl.stream));
        // (byte text: the kept characters are starts[R'], and they lie at the front of the sequence bytes)
        if (sl.h_seq && n_bases) FX_HIP(hipMemcpyAsync(sl.h_seq, sl.d_packed, n_bases, hipMemcpyDeviceToHost, sl.stream));
        if (n_records) FX_HIP(hipMemcpyAsync(sl.h_rec_pos, sl.d_rec_pos, n_records * 8, hipMemcpyDeviceToHost, sl.stream));
        FX_HIP(hipMemcpyAsync(sl.h_rec_base, sl.d_rec_base, (n_records + 1) * 8, hipMemcpyDeviceToHost, sl.stream));
        FX_HIP(hipMemcpyAsync(sl.h_offsets, sl.d_offsets, (n_records + 1) * 8, hipMemcpyDeviceToHost, sl.stream));
        if (n_pos) {
            FX_HIP(hipMemcpyAsync(sl.h_pos, sl.d_pos, n_pos * 4, hipMemcpyDeviceToHost, sl.stream));
            if (sl.d_sk) FX_HIP(hipMemcpyAsync(sl.h_sk, sl.d_sk, n_pos * 4, hipMemcpyDeviceToHost, sl.stream));
            if (sl.d_values)
                FX_HIP(hipMemcpyAsync(sl.h_values, sl.d_values, n_pos * (s->cfg.flags & MM_FASTX_VALUES_U128 ? 16 : 8),
                                      hipMemcpyDeviceToHost, sl.stream));
        }
        FX_HIP(hipEventRecord(sl.ev_done, sl.stream));
        sl.state = kDownloading;
    }
    return MM_OK;
}

int collect_all(mm_fastx_stream *s) {
    for (int i = 0, at = s->oldest; i < s->in_flight; ++i, at = (at + 1) % s->n_slots) {
        const int r = collect(s, s->slots[at], false);
        if (r) return r;
    }
    return MM_OK;
}

// after mm_fastx_stream_finish: the last chunk (the part-filled slot and the tail in front of it), as soon as a slot is free
int launch_final(mm_fastx_stream *s) {
    if (!s->finished || s->final_done || s->format == 0) return MM_OK;
    if (!can_fill(s->slots[s->fill])) return MM_OK;
    s->final_done = true;
    return launch(s, 1);
}

template <class T>
hipError_t dev_alloc(T *&p, uint64_t bytes) {
    return hipMalloc(reinterpret_cast<void **>(&p), bytes ? bytes : 8);
}
template <class T>
hipError_t host_alloc(T *&p, uint64_t bytes) {
    return hipHostMalloc(reinterpret_cast<void **>(&p), bytes ? bytes : 8, hipHostMallocDefault);
}

void destroy_slots(mm_fastx_stream *s) {
    for (int i = 0; i < s->n_slots; ++i) {
        Slot &sl = s->slots[i];
        if (sl.stream) (void)hipStreamSynchronize(sl.stream);
    }
    for (int i = 0; i < s->n_slots; ++i) {
        Slot &sl = s->slots[i];
        void *dev[] = {sl.d_text, sl.d_packed, sl.d_amb, sl.d_rec_base, sl.d_rec_pos, sl.d_offsets, sl.d_meta, sl.d_pos, sl.d_sk, sl.d_values, sl.d_one,
                       sl.d_comp, sl.d_blocks, sl.d_crc, sl.d_status};
        for (void *p : dev)
            if (p) (void)hipFree(p);
        void *host[] = {sl.h_text, sl.h_meta, sl.h_rec_pos, sl.h_rec_base, sl.h_offsets, sl.h_values, sl.h_pos, sl.h_sk, sl.h_one, sl.h_seq,
                        sl.h_comp, sl.h_blocks, sl.h_crc};
        for (void *p : host)
            if (p) (void)hipHostFree(p);
        hipEvent_t ev[] = {sl.ev_cut, sl.ev_run, sl.ev_done, sl.ev_tail};
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (sl.ws) mm_workspace_destroy(sl.ws);
    }
}

// Behind the refusals of the create entries: the device, the stream and its slots.  `text`: a byte-text stream - d_packed
// takes the sequence bytes of a text of 2 * chunk_bytes, and the flags MM_FASTX_TEXT_* add their buffers.
int open_stream(mm_fastx_stream_t **out, const mm_plan_t *plan, const mm::ApiPlanInfo &info, const mm_fastx_stream_config_t &cfg,
                uint32_t value_len, bool text, int values_encoding) {
    const uint32_t flags = cfg.flags;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
        (void)hipGetLastError();
        mm::api_set_last_error("no HIP device visible");
        return MM_ERR_NO_DEVICE;
    }
    if (cfg.device < 0 || cfg.device >= n_dev) return MM_ERR_NO_DEVICE;
    DeviceGuard guard;
    mm_fastx_stream *s = new (std::nothrow) mm_fastx_stream;
    if (!s) return MM_ERR_ALLOC;
    s->plan = plan;
    s->info = info;
    s->cfg = cfg;
    s->text = text;
    s->values_encoding = values_encoding;
    s->value_len = value_len;
    s->C = cfg.chunk_bytes;
    s->A = s->C + ((flags & MM_FASTX_LONG_RECORDS) ? 16 : 0);
    s->max_records = cfg.max_records;
    s->max_positions = (cfg.max_positions == 0 || cfg.max_positions > 2 * s->C) ? 2 * s->C : cfg.max_positions;
    s->packed_cap = text ? 2 * s->C + 64 : ((2 * s->C / 4 + 8 + 3) & ~3ull) + 64;
    s->amb_cap = ((2 * s->C / 8 + 8 + 3) & ~3ull) + 64;
    s->n_slots = cfg.slots ? (int)cfg.slots : 3;
    s->format = cfg.format;  // (MM_FASTX_AUTO = 0: not known yet)
    const uint64_t R = s->max_records, P = s->max_positions;
    const uint64_t per_value = flags & MM_FASTX_VALUES_U128 ? 16 : 8;
    const bool want_values = (flags & (MM_FASTX_VALUES_U64 | MM_FASTX_VALUES_U128)) != 0;
    const bool want_one = (flags & (text ? MM_FASTX_TEXT_ONE_MINIMIZER : MM_FASTX_ONE_MINIMIZER)) != 0, want_seq = text && (flags & MM_FASTX_TEXT_SEQ);
    int rc = MM_OK;
    hipError_t e = hipSetDevice(cfg.device);
    for (int i = 0; i < s->n_slots && e == hipSuccess && rc == MM_OK; ++i) {
        Slot &sl = s->slots[i];
        rc = mm_workspace_create(&sl.ws, cfg.device, nullptr);
        if (rc) break;
        sl.stream = mm::api_workspace_stream(sl.ws);
        e = hipSetDevice(cfg.device);
        if (e == hipSuccess) e = dev_alloc(sl.d_text, s->A + s->C + 64);
        if (e == hipSuccess) e = dev_alloc(sl.d_packed, s->packed_cap);
        if (e == hipSuccess && (flags & MM_FASTX_SKIP_AMBIGUOUS)) e = dev_alloc(sl.d_amb, s->amb_cap);
        if (e == hipSuccess) e = dev_alloc(sl.d_rec_base, (R + 1) * 8);
        if (e == hipSuccess) e = dev_alloc(sl.d_rec_pos, (R + 1) * 8);
        if (e == hipSuccess) e = dev_alloc(sl.d_offsets, (R + 1) * 8);
        if (e == hipSuccess) e = dev_alloc(sl.d_meta, 128);
        if (e == hipSuccess) e = hipMemset(sl.d_meta, 0, 128);
        if (e == hipSuccess) e = dev_alloc(sl.d_pos, P * 4);
        if (e == hipSuccess && (flags & MM_FASTX_SK)) e = dev_alloc(sl.d_sk, P * 4);
        if (e == hipSuccess && want_values) e = dev_alloc(sl.d_values, P * per_value);
        if (e == hipSuccess && want_one) e = dev_alloc(sl.d_one, R * 4);
        if (e == hipSuccess) e = host_alloc(sl.h_text, s->C);
        if (e == hipSuccess) e = host_alloc(sl.h_meta, 128);
        if (e == hipSuccess) e = host_alloc(sl.h_rec_pos, (R + 1) * 8);
        if (e == hipSuccess) e = host_alloc(sl.h_rec_base, (R + 1) * 8);
        if (e == hipSuccess) e = host_alloc(sl.h_offsets, (R + 1) * 8);
        if (e == hipSuccess) e = host_alloc(sl.h_pos, P * 4);
        if (e == hipSuccess && (flags & MM_FASTX_SK)) e = host_alloc(sl.h_sk, P * 4);
        if (e == hipSuccess && want_values) e = host_alloc(sl.h_values, P * per_value);
        if (e == hipSuccess && want_one) e = host_alloc(sl.h_one, R * 4);
        if (e == hipSuccess && want_seq) e = host_alloc(sl.h_seq, 2 * s->C);
        hipEvent_t *ev[] = {&sl.ev_cut, &sl.ev_run, &sl.ev_done, &sl.ev_tail};
        for (hipEvent_t *p : ev)
            if (e == hipSuccess) e = hipEventCreateWithFlags(p, hipEventDisableTiming);
        if (e == hipSuccess) {
            memset(sl.h_meta, 0, 128);
            memcpy(reinterpret_cast<uint8_t *>(sl.h_meta) + 120, ">\n", 2);
        }
    }
    if (rc == MM_OK && e != hipSuccess) {
        mm::api_set_last_error((std::string("mm_fastx_stream_create: ") + hipGetErrorString(e)).c_str());
        (void)hipGetLastError();
        rc = (e == hipErrorOutOfMemory) ? MM_ERR_ALLOC : MM_ERR_HIP;
    }
    if (rc) {
        destroy_slots(s);
        delete s;
        return rc;
    }
    *out = s;
    return MM_OK;
}

int open_bgzf(mm_fastx_stream *s);
int feed_text(mm_fastx_stream *s, const uint8_t *text, uint64_t n_bytes, uint64_t *consumed);

}  // namespace

extern "C" {

int mm_fastx_text_stream_extras(const mm_fastx_stream_t *s, mm_fastx_text_extras_t *out) {
    if (!s || !out) return MM_ERR_NULL;
    if (s->delivered >= 0 && s->text) *out = s->extras;
    else memset(out, 0, sizeof *out);
    return MM_OK;
}

int mm_fastx_stream_one_minimizer(const mm_fastx_stream_t *s, const uint32_t **one_min, uint64_t *n_records) {
    if (!s || !one_min || !n_records) return MM_ERR_NULL;
    const bool have = s->delivered >= 0 && !s->text && s->slots[s->delivered].h_one;
    *one_min = have ? s->slots[s->delivered].h_one : nullptr;
    *n_records = have ? s->slots[s->delivered].h_meta[1] : 0;
    return MM_OK;
}

int mm_fastx_text_stream_create(mm_fastx_stream_t **out, const mm_plan_t *text_plan, const mm_fastx_text_stream_config_t *cfg) {
    if (out) *out = nullptr;
    if (!out || !text_plan || !cfg) return MM_ERR_NULL;
    const mm::ApiPlanInfo info = mm::api_plan_info(text_plan);
    const auto refuse = [](int code, const char *why) {
        mm::api_set_last_error((std::string("mm_fastx_text_stream_create: ") + why).c_str());
        return code;
    };
    if (!info.text) return refuse(MM_ERR_BAD_MODE, "a plan of mm_plan_create: use mm_fastx_stream_create");
    if (cfg->chunk_bytes < 64 || cfg->chunk_bytes >= (1ull << 31) || cfg->max_records >= (1ull << 31)) return MM_ERR_LEN_TOO_LARGE;
    const uint32_t flags = cfg->flags;
    if ((flags & MM_FASTX_SK) && info.mode != MM_MINIMIZERS) return refuse(MM_ERR_BAD_MODE, "MM_FASTX_SK needs a minimizer plan");
    if (flags & (MM_FASTX_SKIP_AMBIGUOUS | MM_FASTX_LONG_RECORDS))
        return refuse(MM_ERR_BAD_MODE, "byte text has neither MM_FASTX_SKIP_AMBIGUOUS nor MM_FASTX_LONG_RECORDS");
    if ((flags & MM_FASTX_VALUES_U64) && (flags & MM_FASTX_VALUES_U128)) return refuse(MM_ERR_BAD_MODE, "both values flags");
    const int enc = cfg->values_encoding;
    if (enc != MM_TEXT_VALUES_BYTES && enc != MM_TEXT_VALUES_DNA)
        return refuse(MM_ERR_BAD_MODE, "values_encoding is MM_TEXT_VALUES_BYTES or MM_TEXT_VALUES_DNA");
    const uint32_t value_len = mm_plan_value_len(text_plan);
    if (flags & (MM_FASTX_VALUES_U64 | MM_FASTX_VALUES_U128)) {
        if (enc == MM_TEXT_VALUES_BYTES && info.canonical_hasher)
            return refuse(MM_ERR_BAD_MODE, "MM_TEXT_VALUES_BYTES with a canonical hasher (general text has no reverse complement)");
        const uint32_t per_word = enc == MM_TEXT_VALUES_BYTES ? 8 : 32;
        if (value_len > ((flags & MM_FASTX_VALUES_U128) ? 2 * per_word : per_word)) return MM_ERR_VALUE_LEN;
    }
    const int refusal = mm::api_text_counts_refusal(text_plan, 2 * cfg->chunk_bytes, cfg->max_records, (flags & MM_FASTX_SK) != 0);
    if (refusal) return refusal;
    if (cfg->format == MM_FASTX_FASTQ) return refuse(MM_ERR_FORMAT, "FASTQ to byte records is not provided");
    if (cfg->format < MM_FASTX_AUTO || cfg->format > MM_FASTX_FASTQ || (cfg->slots != 0 && (cfg->slots < 2 || cfg->slots > 8)) ||
        (flags & ~(127u | MM_FASTX_BGZF_CRC)))
        return refuse(MM_ERR_BAD_MODE, "format is MM_FASTX_AUTO / _FASTA, slots 0 or 2..8, flags MM_FASTX_*");
    mm_fastx_stream_config_t base{};
    base.device = cfg->device, base.format = cfg->format, base.flags = flags, base.slots = cfg->slots;
    base.chunk_bytes = cfg->chunk_bytes, base.max_records = cfg->max_records, base.max_positions = cfg->max_positions;
    base.first_byte = cfg->first_byte;
    return open_stream(out, text_plan, info, base, value_len, true, enc);
}

int mm_debug_fastx_cut(const uint8_t *text, uint64_t n, int format, int last, uint64_t out[3]) {
    if (!out || (!text && n)) return MM_ERR_NULL;
    if (format != MM_FASTX_FASTA && format != MM_FASTX_FASTQ) return MM_ERR_BAD_MODE;
    mm::fastx_cut_host(text, n, format, last ? 1 : 0, out);
    return MM_OK;
}

int mm_debug_fastx_split(const uint8_t *text, uint64_t n, uint32_t l, int last, uint64_t out[4]) {
    if (!out || (!text && n)) return MM_ERR_NULL;
    mm::fastx_split_host(text, n, l, last ? 1 : 0, out);
    return MM_OK;
}

int mm_fastx_stream_pieces(const mm_fastx_stream_t *s, mm_fastx_pieces_t *out) {
    if (!s || !out) return MM_ERR_NULL;
    if (s->delivered >= 0) *out = s->pieces;
    else memset(out, 0, sizeof *out);
    return MM_OK;
}

int mm_fastx_stream_create(mm_fastx_stream_t **out, const mm_plan_t *plan, const mm_fastx_stream_config_t *cfg) {
    if (out) *out = nullptr;
    if (!out || !plan || !cfg) return MM_ERR_NULL;
    const mm::ApiPlanInfo info = mm::api_plan_info(plan);
    if (info.text) return MM_ERR_BAD_MODE;
    if (cfg->chunk_bytes < 64 || cfg->chunk_bytes >= (1ull << 31) || cfg->max_records >= (1ull << 31)) return MM_ERR_LEN_TOO_LARGE;
    const uint32_t flags = cfg->flags;
    if ((flags & MM_FASTX_SK) && (info.mode != MM_MINIMIZERS || (flags & MM_FASTX_SKIP_AMBIGUOUS))) return MM_ERR_BAD_MODE;
    if ((flags & MM_FASTX_SKIP_AMBIGUOUS) && !info.canonical_windows) return MM_ERR_HASHER_NOT_CANONICAL;
    if ((flags & MM_FASTX_VALUES_U64) && (flags & MM_FASTX_VALUES_U128)) return MM_ERR_BAD_MODE;
    const uint32_t value_len = mm_plan_value_len(plan);
    if (((flags & MM_FASTX_VALUES_U64) && value_len > 32) || ((flags & MM_FASTX_VALUES_U128) && value_len > 64)) return MM_ERR_VALUE_LEN;
    const int refusal = mm::api_reads_counts_refusal(plan, 2 * cfg->chunk_bytes, cfg->max_records, (flags & MM_FASTX_SK) != 0,
                                                     (flags & MM_FASTX_SKIP_AMBIGUOUS) != 0);
    if (refusal) return refusal;
    if (cfg->format < MM_FASTX_AUTO || cfg->format > MM_FASTX_FASTQ || (cfg->slots != 0 && (cfg->slots < 2 || cfg->slots > 8)) ||
        (flags & ~(31u | MM_FASTX_ONE_MINIMIZER | MM_FASTX_BGZF_CRC))) {
        mm::api_set_last_error("mm_fastx_stream_create: format is MM_FASTX_AUTO / _FASTA / _FASTQ, slots 0 or 2..8, flags MM_FASTX_*");
        return MM_ERR_BAD_MODE;
    }
    if ((flags & MM_FASTX_ONE_MINIMIZER) && (flags & MM_FASTX_LONG_RECORDS)) {
        mm::api_set_last_error("mm_fastx_stream_create: MM_FASTX_ONE_MINIMIZER with MM_FASTX_LONG_RECORDS: a split record's "
                               "minimizer is not joined across its pieces");
        return MM_ERR_BAD_MODE;
    }
    // (a piece must be able to move past its own overlap: l - 1 bases, up to three bytes each with "\r\n" behind every base)
    if ((flags & MM_FASTX_LONG_RECORDS) && cfg->chunk_bytes < 4ull * (info.k + info.w - 1)) {
        mm::api_set_last_error(("mm_fastx_stream_create: MM_FASTX_LONG_RECORDS needs chunk_bytes >= 4 * (k + w - 1) = " +
                                std::to_string(4ull * (info.k + info.w - 1)))
                                   .c_str());
        return MM_ERR_CAPACITY;
    }
    return open_stream(out, plan, info, *cfg, value_len, false, 0);
}

void mm_fastx_stream_destroy(mm_fastx_stream_t *s) {
    if (!s) return;
    DeviceGuard guard;
    (void)hipSetDevice(s->cfg.device);
    destroy_slots(s);
    delete s;
}

int mm_fastx_stream_feed(mm_fastx_stream_t *s, const uint8_t *text, uint64_t n_bytes, uint64_t *consumed) {
    if (consumed) *consumed = 0;
    if (!s || !consumed || (!text && n_bytes)) return MM_ERR_NULL;
    if (s->failed) return again(s);
    if (s->finished) return fail(s, MM_ERR_BAD_MODE, "mm_fastx_stream_feed: called after mm_fastx_stream_finish");
    if (s->bgzf) return fail(s, MM_ERR_BAD_MODE, "mm_fastx_stream_feed: called after mm_fastx_stream_feed_bgzf (text behind BGZF blocks)");
    DeviceGuard guard;
    FX_HIP(hipSetDevice(s->cfg.device));
    return feed_text(s, text, n_bytes, consumed);
}

int mm_fastx_stream_feed_bgzf(mm_fastx_stream_t *s, const uint8_t *data, uint64_t n_bytes, uint64_t *consumed) {
    if (consumed) *consumed = 0;
    if (!s || !consumed || (!data && n_bytes)) return MM_ERR_NULL;
    if (s->failed) return again(s);
    if (s->finished) return fail(s, MM_ERR_BAD_MODE, "mm_fastx_stream_feed_bgzf: called after mm_fastx_stream_finish");
    DeviceGuard guard;
    FX_HIP(hipSetDevice(s->cfg.device));
    if (!s->bgzf) {
        const int r = open_bgzf(s);
        if (r) return r;
    }
    // (bgzf_partial: the bytes fed last end inside a block; only a call that takes a whole block says otherwise, so a call
    // without bytes in between leaves a truncated file truncated)
    uint64_t at = 0;
    while (at < n_bytes) {
        uint64_t total = 0;
        uint32_t payload_off = 0, comp_len = 0, isize = 0;
        const int m = mm::bgzf_member(data + at, n_bytes - at, &total, &payload_off, &comp_len, &isize);
        if (m > 0) {  // (the rest is the front of a block: the caller feeds it again with what follows)
            s->bgzf_partial = true;
            break;
        }
        *consumed = at;
        if (m == -2)
            return fail(s, MM_ERR_FORMAT, "mm_fastx_stream_feed_bgzf: a gzip member without a BC subfield: plain gzip is one serial stream; "
                                          "recompress with bgzip");
        if (m < 0) return fail(s, MM_ERR_FORMAT, "mm_fastx_stream_feed_bgzf: no BGZF block header where one must stand");
        if (isize > mm::kBgzfMaxIsize) return fail(s, MM_ERR_FORMAT, "mm_fastx_stream_feed_bgzf: ISIZE above 65536");
        if (isize == 0) {  // (the EOF marker, the seams of concatenated files)
            at += total;
            s->bgzf_partial = false;
            continue;
        }
        if (isize > s->C)
            return fail(s, MM_ERR_CAPACITY, "mm_fastx_stream_feed_bgzf: a BGZF block of " + std::to_string(isize) +
                                                " bytes of text, more than chunk_bytes = " + std::to_string(s->C));
        Slot &sl = s->slots[s->fill];
        if (!can_fill(sl)) break;
        if (s->format == 0 || (s->format == MM_FASTX_FASTQ && !s->any_launched && sl.n_new == 0)) {
            // in front of the text (format not known, blank bytes in front of a FASTQ): the block's text through feed's rule.
            // Nothing has been launched, so every slot is free; held blank bytes of a FASTA header's line can push the end
            // of the block's text into the slot behind, which is looked at before a byte is taken.
            if (!can_fill(s->slots[(s->fill + 1) % s->n_slots])) break;
            if (mm::inflate_payload_host(data + at + payload_off, comp_len, s->bgzf_first.data(), isize)) return fail_bgzf(s);
            // (MM_FASTX_BGZF_CRC: a block inflated on the host is checked on the host, by the arithmetic the kernel runs)
            if ((s->cfg.flags & MM_FASTX_BGZF_CRC) &&
                mm::crc32_bytes(0, s->bgzf_first.data(), isize) != mm::bgzf_trailer_crc(data + at, total))
                return fail_crc(s);
            uint64_t took = 0;
            const int r = feed_text(s, s->bgzf_first.data(), isize, &took);
            if (r) return r;
            // (cannot happen: at most chunk_bytes + 64 bytes, and two slots were free)
            if (took != isize) return fail(s, MM_ERR_BAD_MODE, "mm_fastx_stream_feed_bgzf: the stream's first text did not fit two free slots");
            at += total;
            s->bgzf_partial = false;
            continue;
        }
        if (isize > s->C - sl.n_new || comp_len > s->comp_cap - sl.n_comp || sl.n_blk == s->table_max) {
            // (the slot holds something: a block alone always fits an empty slot)
            const int r = launch(s, 0);
            if (r) return r;
            continue;
        }
        memcpy(sl.h_comp + sl.n_comp, data + at + payload_off, comp_len);
        if (sl.h_crc) sl.h_crc[sl.n_blk] = mm::bgzf_trailer_crc(data + at, total);
        mm_bgzf_block_t &b = sl.h_blocks[sl.n_blk++];
        b.comp_off = sl.n_comp, b.comp_len = comp_len, b.isize = isize, b.out_off = sl.n_new;
        sl.n_comp += comp_len;
        sl.n_new += isize;
        sl.n_blk_bytes += isize;
        sl.state = kFilling;
        at += total;
        s->bgzf_partial = false;
        if (sl.n_new == s->C) {
            const int r = launch(s, 0);
            if (r) {
                *consumed = at;
                return r;
            }
        }
    }
    *consumed = at;
    return s->in_flight ? collect_all(s) : (int)MM_OK;
}

}  // extern "C"

namespace {

// BGZF input, first use: the slots' compressed staging buffers (chunk_bytes + 64 KiB: a block's payload is below 64 KiB,
// so a block alone always fits) and block tables
int open_bgzf(mm_fastx_stream *s) {
    s->comp_cap = s->C + 65536;
    s->table_max = s->C / 64 + 16 < 65536 ? s->C / 64 + 16 : 65536;
    s->bgzf_first.resize(mm::kBgzfMaxIsize);
    hipError_t e = hipSuccess;
    for (int i = 0; i < s->n_slots && e == hipSuccess; ++i) {
        Slot &sl = s->slots[i];
        e = host_alloc(sl.h_comp, s->comp_cap);
        if (e == hipSuccess) e = dev_alloc(sl.d_comp, s->comp_cap);
        if (e == hipSuccess) e = host_alloc(sl.h_blocks, s->table_max * sizeof(mm_bgzf_block_t));
        if (e == hipSuccess) e = dev_alloc(sl.d_blocks, s->table_max * sizeof(mm_bgzf_block_t));
        if (e == hipSuccess && (s->cfg.flags & MM_FASTX_BGZF_CRC)) {
            e = host_alloc(sl.h_crc, s->table_max * sizeof(uint32_t));
            if (e == hipSuccess) e = dev_alloc(sl.d_crc, s->table_max * sizeof(uint32_t));
            if (e == hipSuccess) e = dev_alloc(sl.d_status, s->table_max * sizeof(uint32_t));
        }
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(s, e == hipErrorOutOfMemory ? MM_ERR_ALLOC : MM_ERR_HIP, std::string("mm_fastx_stream_feed_bgzf: ") + hipGetErrorString(e));
    }
    s->bgzf = true;
    return MM_OK;
}

// what mm_fastx_stream_feed does behind its refusals (mm_fastx_stream_feed_bgzf: the text of the stream's first blocks)
int feed_text(mm_fastx_stream *s, const uint8_t *text, uint64_t n_bytes, uint64_t *consumed) {
    uint64_t taken = 0;
    // in front of the text: FASTQ has to start with its first '@' (a line's role is the number of newlines in front of it),
    // so blank bytes are passed over and counted; FASTA keeps every byte (what stands in front of a '>' decides about it)
    while (taken < n_bytes && (s->format == 0 || (s->format == MM_FASTX_FASTQ && !s->any_launched && s->slots[s->fill].n_new == 0))) {
        const uint8_t c = text[taken];
        if (is_blank(c)) {
            ++taken, ++s->skipped;
            if (s->format == 0) {
                if (c == '\n') s->line_blanks.clear();
                else if (s->line_blanks.size() < 64) s->line_blanks.push_back((char)c);
            }
            continue;
        }
        if (s->format != 0) break;
        if (c == '@' && s->text) {
            *consumed = taken;
            return fail(s, MM_ERR_FORMAT, "mm_fastx_stream_feed: the first non-blank byte is '@': FASTQ to byte records is not provided");
        } else if (c == '@') {
            s->format = MM_FASTX_FASTQ;
        } else if (c == '>') {
            // (blank lines in front are gone; blank bytes on the header's own line stay, they make it no header)
            s->format = MM_FASTX_FASTA;
            Slot &sl = s->slots[s->fill];
            memcpy(sl.h_text, s->line_blanks.data(), s->line_blanks.size());
            sl.n_new = s->line_blanks.size();
            sl.state = kFilling;
            s->skipped -= s->line_blanks.size();
        } else {
            *consumed = taken;
            return fail(s, MM_ERR_FORMAT, "mm_fastx_stream_feed: the first non-blank byte is neither '@' (FASTQ) nor '>' (FASTA)");
        }
        break;
    }
    while (taken < n_bytes && s->format != 0) {
        Slot &sl = s->slots[s->fill];
        if (!can_fill(sl)) break;
        sl.state = kFilling;
        const uint64_t room = s->C - sl.n_new, m = room < n_bytes - taken ? room : n_bytes - taken;
        memcpy(sl.h_text + sl.n_new, text + taken, m);
        sl.n_new += m;
        taken += m;
        if (sl.n_new == s->C) {
            const int r = launch(s, 0);
            if (r) {
                *consumed = taken;
                return r;
            }
        }
    }
    *consumed = taken;
    return s->in_flight ? collect_all(s) : (int)MM_OK;
}

}  // namespace

extern "C" {

int mm_fastx_stream_finish(mm_fastx_stream_t *s) {
    if (!s) return MM_ERR_NULL;
    if (s->failed) return again(s);
    if (s->bgzf_partial)
        return fail(s, MM_ERR_FORMAT, "mm_fastx_stream_finish: the last mm_fastx_stream_feed_bgzf ended inside a BGZF block (a truncated file)");
    DeviceGuard guard;
    FX_HIP(hipSetDevice(s->cfg.device));
    s->finished = true;
    return launch_final(s);
}

int mm_fastx_stream_next(mm_fastx_stream_t *s, mm_fastx_batch_t *out) {
    if (!s || !out) return MM_ERR_NULL;
    memset(out, 0, sizeof *out);
    if (s->failed) return again(s);
    DeviceGuard guard;
    FX_HIP(hipSetDevice(s->cfg.device));
    if (s->delivered >= 0) {  // the batch handed out by the last call: its slot is free again
        Slot &d = s->slots[s->delivered];
        d.state = kFree;
        clear_new(d);
        s->delivered = -1;
    }
    int r = launch_final(s);
    if (r) return r;
    if (s->in_flight == 0) return s->finished && (s->final_done || s->format == 0) ? (int)MM_FASTX_END : (int)MM_FASTX_NEED_INPUT;
    r = collect_all(s);
    if (r) return r;
    Slot &sl = s->slots[s->oldest];
    const bool must = s->finished || !can_fill(s->slots[s->fill]);
    if (sl.state == kRunning) {
        if (!must) return MM_FASTX_NEED_INPUT;
        r = collect(s, sl, true);
        if (r) return r;
    }
    if (!must) {
        const hipError_t q = hipEventQuery(sl.ev_done);
        if (q == hipErrorNotReady) {
            (void)hipGetLastError();
            return MM_FASTX_NEED_INPUT;
        }
        if (q != hipSuccess) return fail_hip(s, q, "hipEventQuery");
    }
    FX_HIP(hipEventSynchronize(sl.ev_done));
    const uint64_t n_records = sl.h_meta[1];
    for (uint64_t i = 0; i < n_records; ++i) sl.h_rec_pos[i] += sl.abs_begin;
    // The seam (MM_FASTX_LONG_RECORDS), decided here because batches are handed out in the order of the text: a piece's
    // first window always emits its minimizer, so when that is the position the record emitted last (the window before
    // the seam chose it too) the piece's first element is dropped - the batch starts at element 1 and the offsets behind
    // record 0 move down by one.  Syncmers have no such rule: with l - 1 bases repeated no window occurs twice.
    uint64_t drop = 0;
    const bool last_open = long_fasta(s) && !sl.last && sl.h_meta[5];
    memset(&s->pieces, 0, sizeof s->pieces);
    if (!sl.continues) s->have_last = false;
    if ((sl.continues || last_open) && n_records) {
        const uint64_t n0 = sl.h_offsets[1];
        if (sl.continues) {
            if (sl.first_base + (sl.h_rec_base[1] - sl.h_rec_base[0]) >= (1ull << 32))
                return fail(s, MM_ERR_LEN_TOO_LARGE, "mm_fastx_stream: a record of 2^32 bases or more");
            sl.h_rec_pos[0] = sl.rec0_pos;
            if (s->info.mode == MM_MINIMIZERS && n0 && s->have_last && sl.h_pos[0] == s->last_emitted) drop = 1;
            s->pieces.first_continues = 1;
            s->pieces.first_base = sl.first_base;
            s->pieces.first_overlap = sl.first_overlap;
        }
        if (n0) {
            s->have_last = true;
            s->last_emitted = sl.h_pos[n0 - 1];
        }
        if (drop)
            for (uint64_t i = 1; i <= n_records; ++i) --sl.h_offsets[i];
    }
    s->pieces.last_open = last_open ? 1 : 0;
    out->n_records = n_records;
    out->n_bases = sl.h_meta[0];
    out->n_positions = sl.h_meta[7] - drop;
    out->text_begin = sl.report_begin;
    out->text_end = sl.abs_begin + (sl.last ? sl.n_text : sl.h_meta[2]);
    out->rec_text_pos = sl.h_rec_pos;
    out->rec_base = sl.h_rec_base;
    out->offsets = sl.h_offsets;
    out->pos = sl.h_pos + drop;
    out->sk = sl.h_sk ? sl.h_sk + drop : nullptr;
    out->values = sl.h_values ? sl.h_values + drop * (s->cfg.flags & MM_FASTX_VALUES_U128 ? 2 : 1) : nullptr;
    s->extras.one_min = sl.h_one;
    s->extras.seq = sl.h_seq;
    sl.state = kDelivered;
    s->delivered = s->oldest;
    s->oldest = (s->oldest + 1) % s->n_slots;
    --s->in_flight;
    return MM_OK;
}

}  // extern "C"
