/*
 * simd_minimizers_amd.h — C ABI of the MI355X (gfx950) minimizer engine.
 *
 * This is the drop-in boundary for the hot path of rust-seq/simd-minimizers
 * v3.0.0 (packed-seq decode -> ntHash -> sliding-window min -> dedup/collect,
 * the canonical variant, the syncmer filter, super-k-mer indices and k-mer
 * values).  The reference has no FFI of its own: the path sits behind its
 * Rust builder API (src/lib.rs:225-577).  Each entry point below names the
 * reference item it replaces; INTEGRATION.md shows the Rust `extern "C"`
 * binding a maintainer would add.
 *
 * Conventions: plain pointers and sizes, no C++/torch types; every function
 * returns 0 (MM_OK) or a negative MM_ERR_* code and never aborts.  The HIP
 * kernels are the only compute path: there is no CPU fallback.
 *
 * Current device: an entry point selects its workspace's device (a device
 * group's entries one after the other) while it runs and RESTORES the calling
 * thread's current device before it returns - a caller that works with several
 * GPUs finds hipGetDevice() unchanged after every call (round 6).  Device
 * pointers passed in must belong to the device the call works on: a
 * workspace's device, the root entry's device for the gather calls.
 */
#ifndef SIMD_MINIMIZERS_AMD_H
#define SIMD_MINIMIZERS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ types */

/* seq-hash KmerHasher as data (call sites src/minimizers.rs:24,44,61,85,143; src/lib.rs:391).
 *   h_fw(i) = fw_xor ^ XOR_j rotl(fw[s[i+j]], rot*(k-1-j));  h_rc(i) = rc_xor ^ XOR_j rotl(rc[s[i+j]], rot*j)
 *   h = canonical ? h_fw + h_rc (wrapping) : h_fw
 * The tables cross the ABI as data, so a seeded hasher (`new_with_seed`, src/lib.rs:157) or another
 * hasher of this rolling rot-xor form is a parameter and not a rebuild.  fw_xor / rc_xor are constants
 * XORed onto the strand hashes (0 for NtHasher; folded into the kernels' tables, no cost per base);
 * `kind` says which seq-hash type the tables stand for (informational: the kernels only see the
 * tables). */
typedef struct mm_hasher {
    uint32_t fw[4];
    uint32_t rc[4];
    uint32_t rot;
    uint32_t canonical;
    uint32_t fw_xor;
    uint32_t rc_xor;
    uint32_t kind; /* mm_hasher_kind_t */
} mm_hasher_t;

typedef enum mm_hasher_kind { MM_HASHER_NT = 0, MM_HASHER_MUL = 1, MM_HASHER_ANTILEX = 2 } mm_hasher_kind_t;

/* Builder<_, _, _, SYNCMER> (src/lib.rs:221-225): 0 minimizers, 1 closed, 2 open syncmers */
typedef enum mm_mode { MM_MINIMIZERS = 0, MM_CLOSED_SYNCMERS = 1, MM_OPEN_SYNCMERS = 2 } mm_mode_t;

/* Which kernel family a run used (diagnostics; all are HIP kernels).  MM_PATH_SPLIT is the fused family's
 * two-stream form: the same walk, its lists expanded to positions by a second, concurrent kernel. */
typedef enum mm_path { MM_PATH_FUSED = 1, MM_PATH_GENERIC = 2, MM_PATH_SPLIT = 3 } mm_path_t;

typedef struct mm_device_group mm_device_group_t; /* one workspace per listed device (several-device calls) */
typedef struct mm_plan mm_plan_t;           /* immutable (k, w, hasher, mode): the Builder     */
typedef struct mm_workspace mm_workspace_t; /* per-stream device scratch: the thread-local CACHE
                                               of src/lib.rs:217-219, src/collect.rs:124-126   */
/* Threads: one workspace per host thread / stream; plans are immutable and shareable.
 *   - a plan is never written after mm_plan_create*: any number of threads may run with it at once;
 *   - a workspace or a device group is used by ONE thread at a time (no lock inside); it may move from
 *     one thread to another between calls;
 *   - mm_last_error() is per thread: it tells the calling thread about its own last failure;
 *   - an entry point restores the CALLING thread's current device before it returns. */

/* One entry per assert!/panic! on the reference path. */
enum {
    MM_OK = 0,
    MM_ERR_W_ZERO = -1,               /* src/sliding_min.rs:91,227 */
    MM_ERR_W_TOO_LARGE = -2,          /* src/sliding_min.rs:92-95,228 */
    MM_ERR_LEN_TOO_LARGE = -3,        /* src/sliding_min.rs:96-99,229 */
    MM_ERR_EVEN_L = -4,               /* src/canonical.rs:13-16,43-46 */
    MM_ERR_HASHER_NOT_CANONICAL = -5, /* src/minimizers.rs:81,139 */
    MM_ERR_OPEN_EVEN_W = -6,          /* src/syncmers.rs:24-29 */
    MM_ERR_K_ZERO = -7,
    MM_ERR_CAPACITY = -8,             /* caller's output buffer too small; *out_count holds the need */
    MM_ERR_BAD_MODE = -9,             /* src/lib.rs:437; super-k-mers with syncmers, src/lib.rs:339 */
    MM_ERR_NULL = -10,
    MM_ERR_VALUE_LEN = -11,           /* values_u64 needs len <= 32, values_u128 len <= 64; of byte text as `&[u8]`
                                         (MM_TEXT_VALUES_BYTES) len <= 8 and len <= 16 */
    MM_ERR_FORMAT = -12,              /* the text is FASTQ ('@' first), not FASTA (today: mm_fasta_text_device) */
    MM_ERR_NO_DEVICE = -20,           /* no HIP device: the engine has no CPU fallback */
    MM_ERR_HIP = -21,                 /* a HIP call failed; see mm_last_error() */
    MM_ERR_ALLOC = -22,
    MM_ERR_ORDER = -23,               /* mm_workspace_check: a look-back of an asynchronous run timed out */
    MM_ERR_UNSORTED = -24             /* mm_run_text_batch_host: record starts decrease */
};

const char *mm_strerror(int code);
/* Text of the last HIP failure seen by this thread ("" if none). */
const char *mm_last_error(void);
/* Number of visible HIP devices (0 if none; never initialises a device context). */
int mm_device_count(void);

/* ----------------------------------------------------------------- hasher */

/* NtHasher::<CANONICAL>::new(k) (seq-hash 0.2.0; src/lib.rs:391). */
int mm_default_hasher(mm_hasher_t *out, int canonical);
/* MulHasher::<CANONICAL>::new(k) and AntiLexHasher::<CANONICAL>::new(k) (seq-hash 0.2.0; src/lib.rs:71-72,
 * exercised by src/test.rs:81-83,107-109).  PARITY UNPINNED: their arithmetic is not in the reference
 * tree and the reference holds no known-answer vector for them, so these fill the tables with this
 * engine's restatement of the published idea - mulHash: the character value times a pseudo-random
 * constant in NtHasher's rolling form; anti-lex: the k-mer's own base-4 value with the first base
 * inverted - and a caller who has the real crate puts ITS per-base values into mm_hasher_t instead.
 * Everything downstream (windows, ties, strand vote, collectors) is the pinned path. */
int mm_mul_hasher(mm_hasher_t *out, int canonical);
int mm_antilex_hasher(mm_hasher_t *out, uint32_t k, int canonical);

/* ------------------------------------------------------------------- plan */

/* minimizers / canonical_minimizers / closed_syncmers / canonical_closed_syncmers /
 * open_syncmers / canonical_open_syncmers (src/lib.rs:240-321) + .hasher() (:327).
 * `canonical_windows` selects the strand-vote tie-break (src/minimizers.rs:74-166);
 * `hasher == NULL` means H::new(k) with the matching CANONICAL (src/lib.rs:391-394).
 * Validates every precondition the reference asserts and returns the matching error. */
int mm_plan_create(mm_plan_t **out, uint32_t k, uint32_t w, int canonical_windows, mm_mode_t mode,
                   const mm_hasher_t *hasher);
void mm_plan_destroy(mm_plan_t *plan);
/* len of the values: k for minimizers, k+w-1 for syncmers (src/lib.rs:439-447) */
uint32_t mm_plan_value_len(const mm_plan_t *plan);

/* -------------------------------------------------------------- workspace */

/* Device scratch bound to one HIP device and one stream.  `hip_stream` may be NULL
 * (a private stream is created; it is a blocking stream, i.e. ordered against the legacy
 * default stream) or a hipStream_t owned by the caller. */
int mm_workspace_create(mm_workspace_t **out, int device, void *hip_stream);
void mm_workspace_destroy(mm_workspace_t *ws);
int mm_workspace_sync(mm_workspace_t *ws);
/* Status of the ASYNCHRONOUS runs issued on this workspace since the last check (the reference has
 * no counterpart: its calls are synchronous; this is the completion half of the *_async entry
 * points).  Waits for the workspace stream, then returns MM_OK, or
 *   MM_ERR_ORDER  the fused kernel's look-back timed out in one of them (workgroups were not
 *                 dispatched in index order): that run's output and count are invalid; every later
 *                 run on this workspace takes its tile ids from an atomic ticket, so repeating the
 *                 runs issued since the last check gives the right result;
 *   MM_ERR_CAPACITY  mm_run_text_batch_counts_device_async found d_counts beyond max_chars / max_records (an asynchronous
 *                 loader that overflowed its tables): that run wrote count 0 and offsets[0] = 0, nothing else, and its
 *                 values call wrote nothing; mm_last_error() names the call.  Likewise
 *                 mm_run_packed_reads_counts_device_async found d_counts beyond max_bases / max_records: that run wrote
 *                 count 0 and offsets of 0, no position;
 *   MM_ERR_HIP    a kernel refused to run (mm_last_error() says why).
 * The synchronous entry points check (and repeat the run) themselves. */
int mm_workspace_check(mm_workspace_t *ws);
/* Force the generic (any k, any w) kernel family instead of the fused one (testing). */
int mm_workspace_force_generic(mm_workspace_t *ws, int on);
/* Windows per lane of the fused kernel, in units of w (0 = built-in default). Tuning knob. */
int mm_workspace_set_blocks_per_lane(mm_workspace_t *ws, uint32_t nblk);
/* HIP-event timing of the dominant kernel: when enabled every launch of the hot kernel is
 * bracketed by events on the workspace stream; read back the sum and the launch count. */
int mm_workspace_enable_timing(mm_workspace_t *ws, int on);
int mm_workspace_kernel_time(mm_workspace_t *ws, double *total_ms, uint64_t *launches,
                             int reset);
/* Family used by the last run (mm_path_t). */
int mm_workspace_last_path(const mm_workspace_t *ws);
/* 1 once this workspace takes the fused kernels' tile ids from an atomic ticket (after a look-back of one of its
 * runs timed out: workgroups were not dispatched in index order), else 0.  Read-only diagnostic: results are the
 * same either way, the synchronous entry points repeat such a run themselves. */
int mm_workspace_ticket_mode(const mm_workspace_t *ws);
/* 1 when the last reads / batch run on this workspace was a LANE-TABLE launch (round 6): one launch of the reads-mode
 * kernel whose lanes are segments of the reads - a read longer than a lane takes consecutive lanes - so reads and
 * sequences of any lengths (Builder::run per read / contig, src/lib.rs:378; the reference's `short` experiment spans
 * lengths 16 .. 16 384, bench/src/bin/paper.rs:62-115) fill every tile.  mm_run_reads_device*, mm_run_packed_reads_*
 * take it when the longest read exceeds a default lane, mm_run_batch_device for batches of short sequences that lie in
 * ONE device allocation within 2^32 bases of one another (one descriptor then covers them all; sequences in separate
 * allocations keep tiles of their own, whose loads are clamped to each sequence's bytes); diagnostics only, results are
 * the same on every path. */
int mm_workspace_last_lane_table(const mm_workspace_t *ws);
/* Window sizes w for which the library carries a PREBUILT fused kernel (every other w <= 128 is specialised at
 * first use, larger ones take the generic family): canonical_windows 0 / 1 selects the forward / canonical
 * instances, reads_mode 0 / 1 the sequence-mode / reads-mode ones.  Writes up to `capacity` sizes in ascending
 * order to `out` (may be null) and returns how many there are.  No GPU needed.  The test-suite takes its list of
 * instances to compare with the oracle from here, so that none can ship untested. */
int mm_prebuilt_window_sizes(int canonical_windows, int reads_mode, uint32_t *out, int capacity);
/* The same list PER FLAVOUR: `mode` and `super_kmers` (minimizers with super-k-mer indices; 0 sizes with a syncmer mode)
 * select the kernel.  A sequence-mode instance carries all four flavours, so reads_mode == 0 gives the list above for
 * each of them; in reads mode minimizer positions have the list above, and closed syncmers, open syncmers and
 * minimizers + super-k-mers are prebuilt for w = 5, 7, 11, 15, 17, 19, 21, 31.  Every other (flavour, w <= 128) is
 * compiled at its first use - or ahead of it by mm_plan_prepare - which Builder::run (src/lib.rs:378), being compiled
 * code, never is.  A table look-up: no GPU needed, none touched. */
int mm_prebuilt_flavour_window_sizes(int canonical_windows, int reads_mode, mm_mode_t mode, int super_kmers,
                                     uint32_t *out, int capacity);

/* ----------------------------------------------------------- first call */

/* The reference's Builder::run (src/lib.rs:378) is ordinary compiled code: its first call costs what its thousandth
 * does.  Here the first run of a plan loads its kernels onto the device and, for a (flavour, w) without a prebuilt
 * kernel, compiles one with hiprtc - seconds.  mm_plan_prepare restores the reference's behaviour for a caller that
 * wants it: it obtains every kernel the plan's runs can dispatch to under `what`, exactly as their first launch would
 * (the launcher's own choice: fixed-k instance, prebuilt instance, else the run-time compiler and its disk cache), on
 * the workspace's device, and launches nothing; the calling thread's current device is what it was on return.
 *   MM_PREPARE_SEQUENCE    mm_run_device*, mm_run_host*, mm_run_skip_ambiguous_*, tiled mm_run_batch_device launches
 *   MM_PREPARE_READS       mm_run_reads_*, mm_run_packed_reads_* and lane-table launches (with the table's kernels)
 *   MM_PREPARE_SUPERKMERS  also the kernels of the same runs with super-k-mer indices (d_out_sk); MM_ERR_BAD_MODE for a
 *                          syncmer plan, as the runs themselves reject d_out_sk there (src/lib.rs:339)
 * A text plan (mm_plan_create_text) has its fused text kernels - or the generic family's - loaded; none is compiled.
 * report (may be NULL): `kernels` = kernels looked at; of them `compiled` were compiled by hiprtc in this call,
 * `from_disk` were loaded from MM_JIT_CACHE_DIR, `unavailable` cannot be had (MM_JIT=0, a compile failure) -
 * the rest were prebuilt or already loaded.  Runs of a plan with unavailable kernels take the generic family, as they
 * do without prepare: the call still returns MM_OK, loads that family, and mm_last_error() carries the reason.
 * A plan with w > 128 has no fused kernel by design: the prebuilt generic family is its only path, is what gets loaded,
 * and nothing counts as unavailable.
 * After MM_OK with unavailable == 0, no run of this plan in the prepared families on this device compiles anything.
 * what == 0, or MM_PREPARE_SUPERKMERS alone (no family named) on a minimizer plan: MM_OK and a zero report; the
 * syncmer-plan check comes first, so MM_PREPARE_SUPERKMERS alone on a syncmer plan is still MM_ERR_BAD_MODE.  Bits of
 * `what` other than the three above: MM_ERR_BAD_MODE.  MM_ERR_NULL for a null plan or workspace (checked before
 * anything else; the report, when given, is zeroed first).  MM_ERR_HIP when the runtime cannot load a prebuilt kernel
 * (mm_last_error() names the call and the cause). */
typedef struct mm_prepare_report {
    uint32_t kernels, compiled, from_disk, unavailable;
} mm_prepare_report_t;
enum { MM_PREPARE_SEQUENCE = 1, MM_PREPARE_READS = 2, MM_PREPARE_SUPERKMERS = 4 };
int mm_plan_prepare(const mm_plan_t *plan, mm_workspace_t *ws, uint32_t what, mm_prepare_report_t *report);
/* Process-wide counters of the run-time compiler since the library was loaded: out[0] hiprtc compiles, out[1] kernels
 * loaded from the disk cache, out[2] requests answered with a kernel already loaded, out[3] compiles or loads that
 * failed.  Nothing resets them: take differences.  With them a caller can check what Builder::run (src/lib.rs:378)
 * guarantees by construction - that a call compiled nothing.  A request for a loaded kernel never waits for another
 * thread's compile, and different kernels compile side by side.  No GPU needed. */
int mm_jit_stats(uint64_t out[4]);
/* Bytes behind the last base of a run's last window that a launch of the fused family may still TOUCH (never use: a lane
 * that starts inside the window range walks its whole length with the windows past the range masked, and its loads run
 * ahead).  The launcher's own bound: mm_device_group_upload_range keeps that much resident behind every entry's share and
 * mm_run_sharded_device's residency check allows for it.  No GPU needed. */
uint64_t mm_fused_overread_bytes(void);

/* -------------------------------------------------------------------- run */

/* Builder::run on a device-resident PackedSeq (src/lib.rs:378-448, :545-576).
 *
 *  d_packed      device pointer to 2-bit bases, 4 per byte, base i at bits 2(i%4) of byte i/4
 *                (packed-seq PackedSeq), codes A0 C1 T2 G3; any byte alignment
 *  packed_bytes  readable bytes at d_packed (>= ceil((base_offset + n_bases)/4))
 *  base_offset   index of the sequence's first base inside the buffer (PackedSeq slices may
 *                start inside a byte: src/test.rs:42-45)
 *  win_begin/end half-open range of WINDOW indices to produce (0 .. n_bases-l+1); the range
 *                form lets one long sequence be sharded across GPUs with absolute positions and
 *                an exact dedup at the seam (src/collect.rs:265-271).  win_end = UINT64_MAX
 *                means "to the last window".
 *  d_out_pos     device buffer for positions (minimizer modes) / window indices (syncmer modes)
 *  d_out_sk      optional device buffer for super-k-mer start indices (.super_kmers(), :341)
 *  capacity      elements available in d_out_pos (and d_out_sk)
 *  d_count       optional device uint64 receiving the number of outputs
 *
 * Asynchronous on the workspace stream.  Output order equals window order.  Completion status:
 * mm_workspace_check(). */
int mm_run_device_async(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed,
                        uint64_t packed_bytes, uint64_t base_offset, uint64_t n_bases,
                        uint64_t win_begin, uint64_t win_end, uint32_t *d_out_pos,
                        uint32_t *d_out_sk, uint64_t capacity, uint64_t *d_count);

/* Same, then waits and returns the count; MM_ERR_CAPACITY if it exceeded `capacity`. */
int mm_run_device(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed,
                  uint64_t packed_bytes, uint64_t base_offset, uint64_t n_bases,
                  uint64_t win_begin, uint64_t win_end, uint32_t *d_out_pos, uint32_t *d_out_sk,
                  uint64_t capacity, uint64_t *out_count);

/* Builder::run on host memory: H2D copy, kernels, D2H copy (what a Rust caller holding a
 * PackedSeqVec / Vec<u32> binds).  `out_pos == NULL` only counts. */
int mm_run_host(const mm_plan_t *plan, mm_workspace_t *ws, const uint8_t *packed,
                uint64_t base_offset, uint64_t n_bases, uint32_t *out_pos, uint32_t *out_sk,
                uint64_t capacity, uint64_t *out_count);

/* AsciiSeq input (src/lib.rs:92-98): packs (c >> 1) & 3 on the device, then runs. */
int mm_run_host_ascii(const mm_plan_t *plan, mm_workspace_t *ws, const uint8_t *ascii,
                      uint64_t n_bases, uint32_t *out_pos, uint32_t *out_sk, uint64_t capacity,
                      uint64_t *out_count);

/* ------------------------------------------------------------------- text */

/* General byte text, the reference's `&[u8]` input (src/lib.rs:59, :71-72): one character per byte, all 256
 * values legal.  The hasher is mm_hasher_t's rolling rot-xor form with 256-entry tables indexed by the byte:
 *   h_fw(i) = fw_xor ^ XOR_j rotl(fw[s[i+j]], rot*(k-1-j));  h_rc(i) = rc_xor ^ XOR_j rotl(rc[s[i+j]], rot*j)
 *   h = canonical ? h_fw + h_rc (wrapping) : h_fw
 * Canonical windows vote on the bytes themselves: a window is canonical when more than half of its l = k+w-1
 * bytes have bit 1 set (c & 2; src/canonical.rs:26-28 on the characters as a `&[u8]` yields them). */
typedef struct mm_text_hasher {
    uint32_t fw[256];
    uint32_t rc[256];
    uint32_t rot;
    uint32_t canonical;
    uint32_t fw_xor;
    uint32_t rc_xor;
    uint32_t kind; /* mm_hasher_kind_t */
} mm_text_hasher_t;

/* MulHasher::<CANONICAL>::new(k) over bytes (src/lib.rs:71-72: "for `&[u8]`, mulHash is used").
 * PARITY UNPINNED: its arithmetic is not in the reference tree and the reference holds no known-answer vector
 * for it, so this fills the tables with this engine's restatement of the published idea - the character value
 * times a pseudo-random constant, fw[c] = c * 0x9E3779B1, in NtHasher's rolling form - and a caller who has the
 * real crate puts ITS per-byte values into mm_text_hasher_t instead.  rc[c] = comp(c) * 0x9E3779B1 where comp
 * swaps A<->T and C<->G (either case) and keeps every other byte: a complement stated as data, replaceable
 * like the rest of the table. */
int mm_text_mul_hasher(mm_text_hasher_t *out, int canonical);
/* NtHasher (or any 4-symbol hasher) over ASCII DNA (packed-seq AsciiSeq, src/lib.rs:92-98):
 * fw[c] = h->fw[(c >> 1) & 3], rc[c] = h->rc[(c >> 1) & 3]; rot, canonical, fw_xor, rc_xor, kind copied. */
int mm_text_hasher_from_dna(mm_text_hasher_t *out, const mm_hasher_t *h);

/* minimizers / canonical_minimizers / closed_syncmers / open_syncmers ... over `&[u8]` (src/lib.rs:240-321)
 * + .hasher() (:327).  `hasher == NULL` means mm_text_mul_hasher with the matching canonical.  The same
 * precondition checks and error codes as mm_plan_create.  A text plan is accepted by the mm_run_text_*
 * entry points only; every other run entry point returns MM_ERR_BAD_MODE for it, and the text entry points
 * return MM_ERR_BAD_MODE for a plan of mm_plan_create. */
int mm_plan_create_text(mm_plan_t **out, uint32_t k, uint32_t w, int canonical_windows, mm_mode_t mode,
                        const mm_text_hasher_t *hasher);

/* Builder::run on device-resident text (src/lib.rs:378-448).  The contract of mm_run_device_async:
 *  d_text        device pointer to n bytes of text, any alignment
 *  text_bytes    readable bytes at d_text (>= n, else MM_ERR_CAPACITY)
 *  win_begin/end half-open window range (win_end = UINT64_MAX: to the last window), output in window order,
 *                the dedup seam against window win_begin - 1
 *  d_out_pos / d_out_sk / capacity / d_count   as for mm_run_device_async (d_out_pos == NULL counts only)
 * n >= 2^32 returns MM_ERR_LEN_TOO_LARGE before anything is touched.  Kernels: the fused text kernel for
 * w <= 128 and k <= 1024 (one launch; MM_PATH_FUSED), the generic family's text kernels otherwise and under
 * mm_workspace_force_generic (MM_PATH_GENERIC).  The hasher tables travel through a ring of eight page-locked
 * staging slots: a call waits only to reuse a slot whose upload, eight distinct table sets back, is still queued. */
int mm_run_text_device_async(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_text, uint64_t text_bytes,
                             uint64_t n, uint64_t win_begin, uint64_t win_end, uint32_t *d_out_pos,
                             uint32_t *d_out_sk, uint64_t capacity, uint64_t *d_count);
/* Same, then waits and returns the count; MM_ERR_CAPACITY if it exceeded `capacity`. */
int mm_run_text_device(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_text, uint64_t text_bytes,
                       uint64_t n, uint64_t win_begin, uint64_t win_end, uint32_t *d_out_pos, uint32_t *d_out_sk,
                       uint64_t capacity, uint64_t *out_count);
/* Window sizes with a PREBUILT fused text instance (every other w <= 128 runs in the fused kernel's run-time-w
 * instance, larger w in the generic family); the same sizes for canonical_windows 0 and 1.  Writes up to
 * `capacity` sizes in ascending order to `out` (may be null) and returns how many there are.  No GPU needed. */
int mm_text_prebuilt_window_sizes(int canonical_windows, uint32_t *out, int capacity);
/* Builder::run on host text: H2D copy, kernels, D2H copy.  `out_pos == NULL` only counts. */
int mm_run_text_host(const mm_plan_t *plan, mm_workspace_t *ws, const uint8_t *text, uint64_t n,
                     uint32_t *out_pos, uint32_t *out_sk, uint64_t capacity, uint64_t *out_count);

/* Builder::run per record (src/lib.rs:378) over MANY records of byte text in one call: protein databases,
 * proteomes, ORF sets, lines of text.  Record r is the bytes [starts[r], starts[r + 1]) of the text, and its
 * slice out_pos[out_offsets[r] .. out_offsets[r + 1]) is exactly what mm_run_text_host returns for that record
 * alone (likewise out_sk): positions and super-k-mer indices are record-local, the dedup restarts at every record,
 * no window spans two records.  starts is non-decreasing, starts[0] may be above 0; empty records and records
 * shorter than l = k + w - 1 get empty slices.  n_records == 0 is legal (count 0, offsets[0] = 0).
 *  d_text / text_bytes    the text, any alignment; n_chars = d_starts[n_records] (> text_bytes: MM_ERR_CAPACITY)
 *  d_starts               device, [n_records + 1]; unordered starts are the caller's contract breach: the output
 *                         is then undefined, but nothing outside the buffers named here is read or written
 *  d_out_pos (or NULL: count only, offsets still written) / d_out_sk (or NULL) / capacity / d_count
 *                         as for mm_run_text_device_async; d_out_offsets [n_records + 1] is always written
 * n_chars >= 2^32 or n_records >= 2^31 returns MM_ERR_LEN_TOO_LARGE before anything is touched.  Kernels: ONE
 * launch of the fused text kernel (w <= 128, k <= 1024; MM_PATH_FUSED) behind a small launch that finds each
 * tile's records; other plans and mm_workspace_force_generic run one generic-family launch per record
 * (MM_PATH_GENERIC) after copying the starts to the host: correct, but slow - meant for the odd plan, not for
 * throughput. */
int mm_run_text_batch_device_async(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_text,
                                   uint64_t text_bytes, uint64_t n_records,
                                   const uint64_t *d_starts /* [n_records + 1] */, uint64_t n_chars,
                                   uint32_t *d_out_pos, uint32_t *d_out_sk /* or NULL */, uint64_t capacity,
                                   uint64_t *d_out_offsets /* [n_records + 1] */, uint64_t *d_count);
/* Same, then waits and returns the count; MM_ERR_CAPACITY if it exceeded `capacity` (*out_count: the need). */
int mm_run_text_batch_device(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_text, uint64_t text_bytes,
                             uint64_t n_records, const uint64_t *d_starts, uint64_t n_chars, uint32_t *d_out_pos,
                             uint32_t *d_out_sk, uint64_t capacity, uint64_t *d_out_offsets, uint64_t *out_count);
/* The same from HOST memory: one upload of the text (bytes 0 .. starts[n_records]) and the starts, one launch, one
 * download.  Starts that decrease return MM_ERR_UNSORTED before anything is touched. */
int mm_run_text_batch_host(const mm_plan_t *plan, mm_workspace_t *ws, const uint8_t *text, uint64_t n_records,
                           const uint64_t *starts /* host, [n_records + 1] */, uint32_t *out_pos,
                           uint32_t *out_sk /* or NULL */, uint64_t capacity,
                           uint64_t *out_offsets /* [n_records + 1] */, uint64_t *out_count);
/* FASTA text -> records of BYTE text on the device: the loader step in front of the batch calls above and of
 * mm_values_*_text_batch_device_async - a protein FASTA in device memory becomes their d_text / d_starts with no parsing
 * on the CPU.  The reader is mm_fasta_pack_device's (needletail::parse_fastx_file restated as the reference's loader
 * uses it, bench/src/lib.rs:51-82; the crate is not in the reference tree: parity unpinned): a record starts with '>'
 * at the start of a line, its header runs to the end of that line, its sequence is every following line up to the next
 * header line with '\n' and '\r' removed, bytes in front of the first header are ignored.  The sequence bytes are kept
 * AS THEY ARE - no case folding, no alphabet mapping (a text hasher's 256-entry tables do that), any byte value but
 * '\n' / '\r' may occur - and go back to back into d_seq.
 *  d_text / n_bytes        the file's bytes, any alignment; n_bytes >= 2^32 returns MM_ERR_LEN_TOO_LARGE before anything
 *                          is touched
 *  d_seq                   4-byte aligned (MM_ERR_NULL otherwise, like d_packed); seq_capacity_bytes = n_bytes always
 *                          suffices.  d_seq is NOT cleared: exactly the bytes [0, min(characters, seq_capacity_bytes))
 *                          are written, nothing at or beyond that
 *  d_rec_start             [max_records + 1]: record r = bytes [d_rec_start[r], d_rec_start[r + 1]) of d_seq - exactly
 *                          the d_starts of mm_run_text_batch_device_async / mm_values_*_text_batch_device_async
 *  d_rec_text_pos          [max_records] or NULL: byte offset of the record's '>' in the text (the caller slices the
 *                          header from there)
 *  d_counts                [2]: characters (their n_chars), records (their n_records); records past max_records are
 *                          counted but not tabulated
 * An empty text gives counts 0 and d_rec_start[0] = 0.  Everything is queued on the workspace's stream; the caller's
 * current device is restored.  This asynchronous form does NOT look at the first byte: a FASTQ text is read by the
 * FASTA rules (a quality line may begin with '>'), so its records are nonsense - the caller knows its format or uses
 * the synchronous form.  Kernels: the two read passes of the packer (mm_fasta2.hip), the second writing bytes; no
 * limits on line lengths, no order between workgroups, no failure mode of its own. */
int mm_fasta_text_device_async(mm_workspace_t *ws, const uint8_t *d_text, uint64_t n_bytes, uint8_t *d_seq,
                               uint64_t seq_capacity_bytes, uint64_t *d_rec_start /* [max_records + 1] */,
                               uint64_t *d_rec_text_pos /* [max_records] or NULL */, uint64_t max_records,
                               uint64_t *d_counts /* [2]: characters, records */);
/* The same, synchronous: out_counts[0..1] receive the counts.  MM_ERR_CAPACITY when the characters did not fit
 * seq_capacity_bytes or the records did not fit max_records (out_counts holds the true counts: what is needed).
 * MM_ERR_FORMAT when the first non-blank byte is '@': FASTQ to byte records is not provided, and nothing is written. */
int mm_fasta_text_device(mm_workspace_t *ws, const uint8_t *d_text, uint64_t n_bytes, uint8_t *d_seq,
                         uint64_t seq_capacity_bytes, uint64_t *d_rec_start, uint64_t *d_rec_text_pos,
                         uint64_t max_records, uint64_t *d_counts, uint64_t *out_counts /* [2] */);
/* The batch run with its two counts taken from the DEVICE: d_counts has the loader's layout above (d_counts[0] = characters,
 * d_counts[1] = records) and is read when the kernels run, so mm_fasta_text_device_async, this call and
 * mm_values_*_text_batch_counts_device_async queue on one stream and the caller waits once (mm_workspace_check) - file in
 * device memory -> records -> positions -> values with no host wait in between.  The reference has no counterpart: its
 * loader and Builder::run are synchronous host code (bench/src/lib.rs:51-82, src/lib.rs:378).
 *  max_chars / max_records  upper bounds of the two counts, all the host knows: they size the launch.  max_chars >
 *                         text_bytes: MM_ERR_CAPACITY; max_chars >= 2^32 or max_records >= 2^31: MM_ERR_LEN_TOO_LARGE.
 *                         Behind the loader: seq_capacity_bytes and max_records as given to it
 *  d_starts               [max_records + 1]; with (n_chars, n_records) = d_counts[0..1] at kernel time, entries past
 *                         d_starts[n_records] are not read
 *  d_out_pos / d_out_sk / d_out_offsets[0 .. n_records] / d_count
 *                         bit for bit what mm_run_text_batch_device_async writes given n_chars and n_records as host
 *                         arguments; d_out_offsets is [max_records + 1], entries past [n_records] are not written.
 *                         capacity = max_chars always suffices (a window gives at most one position)
 * No window anywhere (n_records == 0, n_chars < l = k + w - 1, max_chars == 0): count 0 and d_out_offsets[0 .. n_records]
 * = 0, written by the kernels.  Counts BEYOND the bounds (d_counts[0] > max_chars or d_counts[1] > max_records): the run
 * writes *d_count = 0 and d_out_offsets[0] = 0, touches nothing else, and mm_workspace_check returns MM_ERR_CAPACITY.  No
 * byte outside [d_text, d_text + text_bytes) is loaded whatever d_counts and d_starts hold.  NULL handling and
 * MM_ERR_BAD_MODE (a packed plan, d_out_sk with syncmers) as for mm_run_text_batch_device_async, in its order; d_counts NULL
 * is MM_ERR_NULL.  Plans the fused text kernel does not take (w > 128, k > 1024) and mm_workspace_force_generic return
 * MM_ERR_BAD_MODE before anything is queued - the generic family's launch per record needs the starts on the host:
 * mm_last_error() points to mm_run_text_batch_device.  Kernels: the launches of mm_run_text_batch_device_async with a grid
 * for max_chars; workgroups past the real tile count leave at once. */
int mm_run_text_batch_counts_device_async(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_text,
                                          uint64_t text_bytes, uint64_t max_chars, uint64_t max_records,
                                          const uint64_t *d_starts /* [max_records + 1] */,
                                          const uint64_t *d_counts /* [2]: characters, records */, uint32_t *d_out_pos,
                                          uint32_t *d_out_sk /* or NULL */, uint64_t capacity,
                                          uint64_t *d_out_offsets /* [max_records + 1] */, uint64_t *d_count);
/* Same, then waits ONCE and returns out[0] = positions, out[1] = n_chars, out[2] = n_records (a look-back time-out repeats
 * the run, as in every synchronous form).  MM_ERR_CAPACITY when the positions exceeded `capacity` (out[0]: the need) or the
 * counts exceeded the bounds (out[0] = 0, out[1..2]: the true counts). */
int mm_run_text_batch_counts_device(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_text, uint64_t text_bytes,
                                    uint64_t max_chars, uint64_t max_records, const uint64_t *d_starts,
                                    const uint64_t *d_counts, uint32_t *d_out_pos, uint32_t *d_out_sk, uint64_t capacity,
                                    uint64_t *d_out_offsets, uint64_t *out /* [3]: positions, n_chars, n_records */);
/* What the kernels of the two calls above make of counts and bounds, by the function they call themselves (no device; for
 * tests): out[0] = real tiles (ceil((n_chars + 1) / 8192); 1 when refused), out[1] = launched tiles (the same of
 * max_chars), out[2] = win_end = n_chars >= l ? n_chars - l + 1 : 0 (l = k + w - 1; 0 when refused), out[3] = 1 when a count
 * exceeds its bound (refused).  The entry points' rule for the bounds: MM_ERR_LEN_TOO_LARGE for max_chars >= 2^32 or
 * max_records >= 2^31; MM_ERR_W_ZERO, MM_ERR_NULL. */
int mm_debug_text_counts_view(uint32_t k, uint32_t w, uint64_t max_chars, uint64_t max_records, uint64_t n_chars,
                              uint64_t n_records, uint64_t out[4]);
/* The per-thread step of that kernel on the host (no device; for tests): the bytes of in[0..32) that `mask` selects
 * (bit i = byte i) moved together to out[0..count), zeros behind them.  Returns the count (MM_ERR_NULL for a null pointer). */
int mm_debug_compact32(const uint8_t in[32], uint32_t mask, uint8_t out[32]);

/* ----------------------------------------------------------------- values */

/* Output::values_u64 (src/lib.rs:584-612): k-mer (minimizers) or l-mer (syncmers) at each
 * position, min(fwd, revcomp) when `canonical`.  Device-resident positions and values. */
int mm_values_u64_device_async(mm_workspace_t *ws, const void *d_packed, uint64_t packed_bytes,
                               uint64_t base_offset, uint64_t n_bases, uint32_t len,
                               int canonical, const uint32_t *d_pos, uint64_t n_pos,
                               uint64_t *d_values);
int mm_values_u64_host(mm_workspace_t *ws, const uint8_t *packed, uint64_t base_offset,
                       uint64_t n_bases, uint32_t len, int canonical, const uint32_t *pos,
                       uint64_t n_pos, uint64_t *values);

/* Output::values_u128 (src/lib.rs:587-629): len <= 64; value i is stored little-endian as
 * values[2i] (low 64 bits) and values[2i+1] (high 64 bits). */
int mm_values_u128_device_async(mm_workspace_t *ws, const void *d_packed, uint64_t packed_bytes,
                                uint64_t base_offset, uint64_t n_bases, uint32_t len,
                                int canonical, const uint32_t *d_pos, uint64_t n_pos,
                                uint64_t *d_values);
int mm_values_u128_host(mm_workspace_t *ws, const uint8_t *packed, uint64_t base_offset,
                        uint64_t n_bases, uint32_t len, int canonical, const uint32_t *pos,
                        uint64_t n_pos, uint64_t *values);

/* Output::values_u64 / values_u128 (src/lib.rs:584-629) of EVERY read of one packed buffer in one launch: what a
 * loop over Builder::run (src/lib.rs:378) and Output::values_* per read computes.  The inputs are what the reads entry
 * points (mm_run_reads_*, mm_run_packed_reads_*) take and write:
 *   d_packed / packed_bytes / base_offset   the packed buffer; no byte outside it is loaded, whatever d_pos holds
 *   n_reads, and the layout: d_read_starts [n_reads + 1] (device; read r starts at base d_read_starts[r], the
 *                            mm_run_packed_reads_* layout), or NULL and read_stride (read r starts at base
 *                            r * read_stride, a 64-bit product: the mm_run_reads_* layout)
 *   d_pos                    the read-local positions, back to back (any 4-byte boundary)
 *   d_out_offsets [n_reads + 1]   as the reads entry points write them: value i belongs to the read r with
 *                            d_out_offsets[r] <= i < d_out_offsets[r + 1] (empty reads are skipped) and is the k-mer
 *                            at base base_offset + start(r) + d_pos[i] of the buffer (64-bit: a read may start at or
 *                            beyond base 2^32); a position with pos + len past its read's end gives an unspecified value
 *   n_pos_max                what d_pos and d_values hold; the TRUE count is d_out_offsets[n_reads], read on the
 *                            device: values at or past it (or past n_pos_max) are not written, so the call can be
 *                            queued behind the packer and the reads run on one stream with no host wait
 *   d_values                 8-byte aligned; u64: n_pos_max words, u128: 2 * n_pos_max words ({lo, hi} per value)
 * len / canonical as for mm_values_u64_device_async (len = mm_plan_value_len).  MM_ERR_NULL for a NULL workspace, and for
 * NULL d_packed / d_pos / d_out_offsets / d_values when there is work; MM_ERR_VALUE_LEN for len == 0, len > 32 (u64) or
 * len > 64 (u128); MM_ERR_CAPACITY when base_offset, or a fixed-stride layout's last read, starts past packed_bytes;
 * n_reads == 0 or n_pos_max == 0 returns MM_OK with nothing launched.  mm_run_batch_device's separately allocated
 * sequences have their own call, mm_values_u64_batch_device_async below; byte text has mm_values_u64_text_device_async
 * and mm_values_u64_text_batch_device_async. */
int mm_values_u64_reads_device_async(mm_workspace_t *ws, const void *d_packed, uint64_t packed_bytes,
                                     uint64_t base_offset, uint64_t n_reads,
                                     const uint64_t *d_read_starts /* [n_reads + 1] or NULL */, uint32_t read_stride,
                                     uint32_t len, int canonical, const uint32_t *d_pos,
                                     const uint64_t *d_out_offsets /* [n_reads + 1] */, uint64_t n_pos_max,
                                     uint64_t *d_values);
int mm_values_u128_reads_device_async(mm_workspace_t *ws, const void *d_packed, uint64_t packed_bytes,
                                      uint64_t base_offset, uint64_t n_reads,
                                      const uint64_t *d_read_starts /* [n_reads + 1] or NULL */, uint32_t read_stride,
                                      uint32_t len, int canonical, const uint32_t *d_pos,
                                      const uint64_t *d_out_offsets /* [n_reads + 1] */, uint64_t n_pos_max,
                                      uint64_t *d_values);
/* The same from HOST memory (Output::values_* per read, src/lib.rs:584-629, of a loop over Builder::run,
 * src/lib.rs:378): one upload of the packed bytes, the starts, the positions and the offsets, one launch, one download
 * of offsets[n_reads] values.  Starts or offsets that decrease return MM_ERR_UNSORTED before anything is touched;
 * MM_ERR_CAPACITY when read_starts[n_reads] (or a fixed-stride layout's last read) lies past packed_bytes. */
int mm_values_u64_reads_host(mm_workspace_t *ws, const uint8_t *packed, uint64_t packed_bytes, uint64_t base_offset,
                             uint64_t n_reads, const uint64_t *read_starts /* [n_reads + 1] or NULL */,
                             uint32_t read_stride, uint32_t len, int canonical, const uint32_t *pos,
                             const uint64_t *offsets /* [n_reads + 1] */, uint64_t *values);
int mm_values_u128_reads_host(mm_workspace_t *ws, const uint8_t *packed, uint64_t packed_bytes, uint64_t base_offset,
                              uint64_t n_reads, const uint64_t *read_starts /* [n_reads + 1] or NULL */,
                              uint32_t read_stride, uint32_t len, int canonical, const uint32_t *pos,
                              const uint64_t *offsets /* [n_reads + 1] */, uint64_t *values);
/* Diagnostics of the reads values kernels (Output::values_*, src/lib.rs:584-629, per read of src/lib.rs:378; no device
 * needed).  mm_debug_values_read_of runs the kernel's read lookup on the host: out_read[j] = the largest r in
 * [0, n_reads] with offsets[r] <= idx[j], -1 if there is none.  mm_values_reads_lds_stage: the number of offsets a
 * workgroup stages in LDS; a workgroup whose values span more reads searches global memory instead. */
int mm_debug_values_read_of(const uint64_t *offsets /* [n_reads + 1] */, uint64_t n_reads, const uint64_t *idx,
                            uint64_t n, int64_t *out_read);
uint32_t mm_values_reads_lds_stage(void);

/* ------------------------------------------------- one minimizer per record */

/* one_minimizer(seq, hasher) (src/minimizers.rs:22-28, re-exported at src/lib.rs:211) of EVERY record of a batch in one
 * call: out[r] is the smallest p in [0, len_r - k] whose h(p) & 0xffff0000 is minimal over the k-mers of record r - the
 * leftmost position of the minimal masked hash.  h is the hasher as mm_hasher_t / mm_text_hasher_t define it, the
 * canonical sum h_fw + h_rc when hasher->canonical is set.  Positions are record-local.
 *   - A record with len_r < k - the empty record included - gets MM_NO_MINIMIZER.  The reference's unwrap() panics there
 *     (src/minimizers.rs:27); in a batch short records are data, not an error.  The value differs from the reference's
 *     SKIPPED (u32::MAX - 1).
 *   - There is NO strand vote: the reference has no one_canonical_minimizer (FIXME at src/minimizers.rs:30), so a canonical
 *     hasher only changes the hash.
 * k is a run-time value (any k >= 1, no plan); uses: bucketing reads by their minimizer, assigning super-k-mers, unitigs or
 * query k-mers to a partition, one anchor per protein.
 *
 * mm_one_minimizer_reads_device_async: the two layouts of mm_values_u64_reads_device_async.
 *   d_packed / packed_bytes / base_offset   the packed buffer (any alignment); no byte outside it is loaded
 *   d_read_starts [n_reads + 1] (device)    read r = bases [starts[r], starts[r + 1]) from base_offset - what
 *                                           mm_fasta_pack_device and mm_fastq_pack_device_async write; or NULL:
 *   read_stride / read_len                  read r = the read_len bases at r * read_stride (a 64-bit product),
 *                                           read_len <= read_stride (else MM_ERR_BAD_MODE); ignored with starts
 *   d_out_pos [n_reads]                     exactly n_reads words are written
 * mm_one_minimizer_text_batch_device_async: records of byte text in the mm_run_text_batch_device_async layout (what
 * mm_fasta_text_device writes); the 256-entry tables travel as the text runs' tables do (a ring of page-locked slots).
 * Checks, in this order: MM_ERR_NULL (workspace, hasher, a buffer or output needed for n_reads > 0), MM_ERR_K_ZERO, then the
 * layout: MM_ERR_LEN_TOO_LARGE (n_reads >= 2^32; host forms: a record of 2^32 - 1 symbols or more), MM_ERR_CAPACITY
 * (base_offset, a fixed-stride layout's last read or - host forms - starts[n] past the buffer), MM_ERR_UNSORTED (host forms:
 * decreasing starts).  n_reads == 0 returns MM_OK with nothing launched.  Device forms: unordered starts are the caller's
 * breach - the output is then undefined, but nothing outside the buffers named here is read or written.  n_reads comes from
 * the host here; the *_counts_* forms below read it on the device.  Every call runs on the workspace's stream and restores the caller's current device;
 * results are valid after mm_workspace_sync.  Kernels (mm_one_min.hip): a fill of one 64-bit key per record, one workgroup
 * per mm_one_minimizer_tile() k-mer start positions that ends in one 64-bit atomic minimum per (tile, record) pair, and a
 * small kernel that turns keys into positions. */
#define MM_NO_MINIMIZER 0xFFFFFFFFu
int mm_one_minimizer_reads_device_async(mm_workspace_t *ws, const mm_hasher_t *hasher, uint32_t k, const void *d_packed,
                                        uint64_t packed_bytes, uint64_t base_offset, uint64_t n_reads,
                                        const uint64_t *d_read_starts /* [n_reads + 1] or NULL */, uint32_t read_stride,
                                        uint32_t read_len, uint32_t *d_out_pos /* [n_reads] */);
int mm_one_minimizer_text_batch_device_async(mm_workspace_t *ws, const mm_text_hasher_t *hasher, uint32_t k,
                                             const void *d_text, uint64_t text_bytes, uint64_t n_records,
                                             const uint64_t *d_starts /* [n_records + 1] */,
                                             uint32_t *d_out_pos /* [n_records] */);
/* The same with the two counts read on the DEVICE, so that the call queues behind a loader with no host wait (the reference
 * has no counterpart: one_minimizer, src/minimizers.rs:22-28, is synchronous host code over one sequence).
 *   d_counts [2] (device)      {symbols, records} in the loaders' layout (mm_fasta_text_device_async; the packers'
 *                              mm_fasta_pack_device_async / mm_fastq_pack_device_async: bases, records), read at kernel time
 *   max_chars / max_bases      bound of d_counts[0]: sizes the grid; max_chars <= text_bytes, base_offset + max_bases inside
 *                              the packed buffer
 *   max_records                bound of d_counts[1]: d_starts holds max_records + 1 words, d_out_pos max_records words
 * With (n_sym, n) = d_counts[0 .. 1]: d_out_pos[0 .. n) is bit for bit what the host-n call above writes for n_reads = n on
 * a buffer cut at n_sym symbols (no symbol at or past min(starts[n], n_sym) is loaded), d_out_pos[n .. max_records) is
 * MM_NO_MINIMIZER, nothing at or past max_records is written.  Counts beyond a bound (n_sym > max_chars, n > max_records):
 * every d_out_pos[0 .. max_records) is MM_NO_MINIMIZER, the starts are not read, and mm_workspace_check returns
 * MM_ERR_CAPACITY once (kernel error 8, raised in the workspace's sticky error word as 6 and 7 are by the counts runs); the
 * workspace stays usable.  The packed form takes the starts layout only (the fixed-stride layout has no loader behind it).
 * Checks, in this order: MM_ERR_NULL (workspace, hasher, d_counts; for max_records > 0 the starts, the output and a buffer
 * when the bound is not 0), MM_ERR_K_ZERO, [max_records == 0: MM_OK, nothing launched], MM_ERR_LEN_TOO_LARGE (max_chars /
 * max_bases >= 2^32, max_records >= 2^31), MM_ERR_CAPACITY (max_chars > text_bytes; base_offset + max_bases past the packed
 * buffer).  Kernels: the same per-tile code, instantiated with the counts read by thread 0 of each workgroup
 * (one_min_counts_view, mm_one_min.h); workgroups past the real last tile leave at once. */
int mm_one_minimizer_text_batch_counts_device_async(mm_workspace_t *ws, const mm_text_hasher_t *hasher, uint32_t k,
                                                    const void *d_text, uint64_t text_bytes, uint64_t max_chars,
                                                    uint64_t max_records, const uint64_t *d_starts /* [max_records + 1] */,
                                                    const uint64_t *d_counts /* [2]: characters, records */,
                                                    uint32_t *d_out_pos /* [max_records] */);
int mm_one_minimizer_reads_counts_device_async(mm_workspace_t *ws, const mm_hasher_t *hasher, uint32_t k, const void *d_packed,
                                               uint64_t packed_bytes, uint64_t base_offset, uint64_t max_bases,
                                               uint64_t max_records, const uint64_t *d_read_starts /* [max_records + 1] */,
                                               const uint64_t *d_counts /* [2]: bases, records */,
                                               uint32_t *d_out_pos /* [max_records] */);
/* ---- One minimizer per read that SKIPS ambiguous bases (N): k-mer-level skipping.  The reference has no counterpart:
 * one_minimizer takes a plain Seq (src/minimizers.rs:22-28), which has no N.  For record r with bases [s_r, e_r) and the
 * ambiguity bits the N packers write (mm_fastq_pack_n_device_async, mm_fasta_pack_n_device_async):
 *   - a k-mer start p in [0, len_r - k] is CLEAN when none of the bases s_r + p .. s_r + p + k - 1 has its bit set;
 *   - out[r] is the smallest clean p whose h(p) & 0xffff0000 is minimal over the clean p of record r;
 *   - out[r] is MM_NO_MINIMIZER when the record has no clean k-mer: len_r < k, a record that is all N, a record in which
 *     every clean run is shorter than k;
 *   - h is exactly the plain call's hash (the canonical sum with a canonical hasher, no strand vote);
 *   - bits outside [s_r, e_r) never influence record r: a neighbour's N, junk in front of the first record or behind the
 *     last;
 *   - with all bits clear the result is bit for bit the plain call's.
 * (A window-level rule - skip the window len - k + 1 when it holds an N - would give MM_NO_MINIMIZER to every read with one
 * N: useless for bucketing.)
 *   d_amb / amb_bytes / amb_offset   bit numbering of mm_run_packed_reads_skip_ambiguous_device_async: base j of the run,
 *                                    counted from base_offset, is bit amb_offset + j; bit i is bit i % 8 of byte i / 8.  No
 *                                    byte outside [d_amb, d_amb + amb_bytes) is loaded: a k-mer that reaches past the packed
 *                                    buffer OR past the bits (8 * amb_bytes - amb_offset of them) does not exist.
 * Everything else - layouts, output, stream, the counts form's contract (kernel error 8, MM_NO_MINIMIZER at and past n, the
 * refusal of counts beyond the bounds) - is word for word the plain forms'.  Checks: the plain forms' in their order, with
 * MM_ERR_NULL for a NULL d_amb where a NULL packed buffer is refused, MM_ERR_CAPACITY for amb_offset > 8 * amb_bytes behind
 * the base_offset check, and in the counts form MM_ERR_CAPACITY for amb_offset + max_bases > 8 * amb_bytes.  Kernels: the
 * same per-tile code instantiated with the tile's ambiguity bits staged in LDS next to its symbols; a lane carries the
 * length of the clean run that ends at its newest symbol (mm_one_min.h). */
int mm_one_minimizer_reads_skip_ambiguous_device_async(mm_workspace_t *ws, const mm_hasher_t *hasher, uint32_t k,
                                                       const void *d_packed, uint64_t packed_bytes, uint64_t base_offset,
                                                       const void *d_amb, uint64_t amb_bytes, uint64_t amb_offset, uint64_t n_reads,
                                                       const uint64_t *d_read_starts /* [n_reads + 1] or NULL */,
                                                       uint32_t read_stride, uint32_t read_len, uint32_t *d_out_pos /* [n_reads] */);
int mm_one_minimizer_reads_skip_ambiguous_counts_device_async(mm_workspace_t *ws, const mm_hasher_t *hasher, uint32_t k,
                                                              const void *d_packed, uint64_t packed_bytes, uint64_t base_offset,
                                                              const void *d_amb, uint64_t amb_bytes, uint64_t amb_offset,
                                                              uint64_t max_bases, uint64_t max_records,
                                                              const uint64_t *d_read_starts /* [max_records + 1] */,
                                                              const uint64_t *d_counts /* [2]: bases, records */,
                                                              uint32_t *d_out_pos /* [max_records] */);
int mm_one_minimizer_reads_skip_ambiguous_host(mm_workspace_t *ws, const mm_hasher_t *hasher, uint32_t k, const uint8_t *packed,
                                               uint64_t packed_bytes, uint64_t base_offset, const uint8_t *amb, uint64_t amb_bytes,
                                               uint64_t amb_offset, uint64_t n_reads,
                                               const uint64_t *read_starts /* [n_reads + 1] or NULL */, uint32_t read_stride,
                                               uint32_t read_len, uint32_t *out_pos /* [n_reads] */);
/* The same from HOST memory: one upload (the bytes and the starts), the launches, one download; they wait. */
int mm_one_minimizer_reads_host(mm_workspace_t *ws, const mm_hasher_t *hasher, uint32_t k, const uint8_t *packed,
                                uint64_t packed_bytes, uint64_t base_offset, uint64_t n_reads,
                                const uint64_t *read_starts /* [n_reads + 1] or NULL */, uint32_t read_stride,
                                uint32_t read_len, uint32_t *out_pos /* [n_reads] */);
int mm_one_minimizer_text_batch_host(mm_workspace_t *ws, const mm_text_hasher_t *hasher, uint32_t k, const uint8_t *text,
                                     uint64_t text_bytes, uint64_t n_records, const uint64_t *starts /* [n_records + 1] */,
                                     uint32_t *out_pos /* [n_records] */);
/* K-mer start positions one workgroup covers (tests place their boundaries by it). */
uint32_t mm_one_minimizer_tile(void);
/* The kernel's own per-tile function on the host, tile after tile, the per-tile keys combined by minimum (no device; for
 * tests).  `tile` overrides the tile size (0: mm_one_minimizer_tile()).  The host forms' checks and codes, minus the
 * workspace. */
int mm_debug_one_minimizer_reads(const mm_hasher_t *hasher, uint32_t k, const uint8_t *packed, uint64_t packed_bytes,
                                 uint64_t base_offset, uint64_t n_reads, const uint64_t *read_starts, uint32_t read_stride,
                                 uint32_t read_len, uint32_t tile, uint32_t *out_pos);
int mm_debug_one_minimizer_text_batch(const mm_text_hasher_t *hasher, uint32_t k, const uint8_t *text, uint64_t text_bytes,
                                      uint64_t n_records, const uint64_t *starts, uint32_t tile, uint32_t *out_pos);
int mm_debug_one_minimizer_reads_skip_ambiguous(const mm_hasher_t *hasher, uint32_t k, const uint8_t *packed, uint64_t packed_bytes,
                                                uint64_t base_offset, const uint8_t *amb, uint64_t amb_bytes, uint64_t amb_offset,
                                                uint64_t n_reads, const uint64_t *read_starts, uint32_t read_stride,
                                                uint32_t read_len, uint32_t tile, uint32_t *out_pos);
/* The counts forms on the host (no device; for tests).  mm_debug_one_minimizer_counts_view: the function every workgroup
 * turns {counts, bounds} into what it works on with - out = {n, limit, refused}; `starts` is read at [n] only, and not at
 * all for a refused view or n == 0 (it may then be NULL).  The two runs: the per-tile function with the view's (n, limit),
 * out_pos[0 .. max_records) as the device forms write it; their checks and codes minus the workspace, and MM_ERR_CAPACITY -
 * the output written all the same - for a refused view (what mm_workspace_check reports behind the device forms). */
int mm_debug_one_minimizer_counts_view(uint64_t max_sym, uint64_t max_records, uint64_t n_sym, uint64_t n,
                                       const uint64_t *starts, uint64_t out[3]);
int mm_debug_one_minimizer_text_batch_counts(const mm_text_hasher_t *hasher, uint32_t k, const uint8_t *text,
                                             uint64_t text_bytes, uint64_t max_chars, uint64_t max_records,
                                             const uint64_t *starts, const uint64_t *counts /* [2], host */, uint32_t tile,
                                             uint32_t *out_pos /* [max_records] */);
int mm_debug_one_minimizer_reads_counts(const mm_hasher_t *hasher, uint32_t k, const uint8_t *packed, uint64_t packed_bytes,
                                        uint64_t base_offset, uint64_t max_bases, uint64_t max_records,
                                        const uint64_t *read_starts, const uint64_t *counts /* [2], host */, uint32_t tile,
                                        uint32_t *out_pos /* [max_records] */);
int mm_debug_one_minimizer_reads_skip_ambiguous_counts(const mm_hasher_t *hasher, uint32_t k, const uint8_t *packed,
                                                       uint64_t packed_bytes, uint64_t base_offset, const uint8_t *amb,
                                                       uint64_t amb_bytes, uint64_t amb_offset, uint64_t max_bases,
                                                       uint64_t max_records, const uint64_t *read_starts,
                                                       const uint64_t *counts /* [2], host */, uint32_t tile,
                                                       uint32_t *out_pos /* [max_records] */);

/* Output::values_u64 / values_u128 (src/lib.rs:584-629) of EVERY sequence of a device batch in one launch: what the loop
 * over the contigs (bench/src/bin/paper.rs:410-431: Builder::run per sequence) and Output::values_* per sequence computes,
 * in place of one mm_values_*_device_async call per sequence.  The inputs are what mm_run_batch_device takes and returns;
 * every array but d_pos and d_values is a HOST array:
 *   n_seqs, d_packed [n_seqs], packed_bytes [n_seqs], base_offsets [n_seqs] or NULL, n_bases [n_seqs]
 *                            the sequences as mm_run_batch_device took them: separate device buffers at any byte
 *                            alignment, in any address order, any distance apart
 *   d_pos                    the sequence-local positions, back to back (device; any 4-byte boundary)
 *   offsets [n_seqs + 1]     as mm_run_batch_device wrote them (offsets[0] == 0): value i belongs to the sequence s with
 *                            offsets[s] <= i < offsets[s + 1] and is the k-mer at base base_offsets[s] + d_pos[i] of
 *                            d_packed[s]; the count is offsets[n_seqs]
 *   d_values                 device, 8-byte aligned; u64: offsets[n_seqs] words, u128: twice that ({lo, hi} per value);
 *                            nothing past them is written
 * len / canonical as for mm_values_u64_device_async (len = mm_plan_value_len).  No byte outside [d_packed[s], d_packed[s] +
 * packed_bytes[s]) is loaded, whatever d_pos holds: a position with pos + len > n_bases[s] gives the value of the sequence's
 * bytes zero-extended past packed_bytes[s], and otherwise whatever the bytes hold.  A sequence without values is never
 * dereferenced: its pointer may be NULL and its packed_bytes 0.
 * The kernel is queued on the workspace's stream and the call does not wait for it; the host arrays are the caller's again
 * on return (the tables are staged through two page-locked areas of the workspace's own, used in turn: a call waits only to
 * reuse an area whose upload, two calls back, is still queued).
 * Refused before anything is touched: MM_ERR_NULL for a NULL workspace, for NULL arrays when there is work and for a NULL
 * d_packed[s] of a sequence that has values; MM_ERR_VALUE_LEN for len == 0, len > 32 (u64) or len > 64 (u128);
 * MM_ERR_UNSORTED for offsets that decrease; MM_ERR_CAPACITY for a sequence with values whose (base_offset + n_bases + 3) / 4
 * exceeds its packed_bytes; MM_ERR_LEN_TOO_LARGE for n_seqs >= 2^32.  n_seqs == 0 or offsets[n_seqs] == 0 returns MM_OK with
 * nothing launched.  Byte text: mm_values_u64_text_device_async / mm_values_u64_text_batch_device_async below. */
int mm_values_u64_batch_device_async(mm_workspace_t *ws, uint64_t n_seqs, const void *const *d_packed,
                                     const uint64_t *packed_bytes, const uint64_t *base_offsets /* or NULL */,
                                     const uint64_t *n_bases, uint32_t len, int canonical, const uint32_t *d_pos,
                                     const uint64_t *offsets /* host, [n_seqs + 1] */, uint64_t *d_values);
int mm_values_u128_batch_device_async(mm_workspace_t *ws, uint64_t n_seqs, const void *const *d_packed,
                                      const uint64_t *packed_bytes, const uint64_t *base_offsets /* or NULL */,
                                      const uint64_t *n_bases, uint32_t len, int canonical, const uint32_t *d_pos,
                                      const uint64_t *offsets /* host, [n_seqs + 1] */, uint64_t *d_values);
/* Diagnostics of the batch values kernels (Output::values_*, src/lib.rs:584-629, per sequence of the loop
 * bench/src/bin/paper.rs:410-431; no device needed).  mm_values_batch_lds_stage: the entries (an offset and a 32-byte
 * sequence descriptor each) a workgroup stages in LDS; a workgroup whose values span more sequences searches global memory
 * instead.  mm_debug_values_batch_view: the view the host derives for one sequence at device address `address`, out6 =
 * {address rounded down to a dword, byte_lo, byte_hi, q_lo, q_hi, base0}: bytes [byte_lo, byte_hi) of the rounded address are
 * the sequence's, dwords [q_lo, q_hi) lie wholly inside them, base0 = base_offset + 4 * byte_lo. */
uint32_t mm_values_batch_lds_stage(void);
int mm_debug_values_batch_view(uint64_t address, uint64_t packed_bytes, uint64_t base_offset, uint64_t out6[6]);

/* Output::values_u64 / values_u128 (src/lib.rs:584-629) of BYTE TEXT, at the positions the mm_run_text_* entry points
 * write.  `encoding` names the reference Seq the text stands for:
 *   MM_TEXT_VALUES_BYTES  `&[u8]` (src/lib.rs:59-60), 8 bits per character: value = sum over j < len of text[p + j] << 8j
 *                         (first character in the low byte); len <= 8 (u64) / 16 (u128), else MM_ERR_VALUE_LEN;
 *                         canonical != 0 is MM_ERR_BAD_MODE (general text has no reverse complement).
 *                         PARITY UNPINNED: layout inferred - packed-seq is not in the reference tree.
 *   MM_TEXT_VALUES_DNA    packed-seq AsciiSeq (src/lib.rs:59, :85-100), 2 bits per character, code(c) = (c >> 1) & 3:
 *                         fwd = sum code(text[p + j]) << 2j, rc = sum (code(text[p + len - 1 - j]) ^ 2) << 2j, value =
 *                         canonical ? min(fwd, rc) : fwd; len <= 32 (u64) / 64 (u128).  Bit for bit what
 *                         mm_values_u64_device_async / mm_values_u128_device_async return on
 *                         PackedSeqVec::from_ascii(text) at the same positions, without the packed copy.
 * Any other encoding: MM_ERR_BAD_MODE.  len = mm_plan_value_len(plan); u128 values are stored {lo, hi}. */
#define MM_TEXT_VALUES_BYTES 0
#define MM_TEXT_VALUES_DNA 1
/* A single text: the contract of mm_values_u64_device_async, on bytes.  d_text: n characters at any alignment, text_bytes
 * readable bytes (n > text_bytes: MM_ERR_CAPACITY; n >= 2^32: MM_ERR_LEN_TOO_LARGE); d_pos: n_pos ABSOLUTE text positions,
 * as mm_run_text_device_async writes them (also for a window range); d_values: 8-byte aligned, n_pos words (u128: twice
 * that).  n_pos == 0 returns MM_OK with nothing launched.  No byte outside [d_text, d_text + text_bytes) is loaded whatever
 * d_pos holds: a k-mer that reaches past text_bytes gets the missing characters as byte 0.  MM_ERR_NULL for a NULL
 * workspace (first, whatever else is wrong) and for NULL arrays when there is work; MM_ERR_VALUE_LEN for len == 0.  The
 * caller's current device is restored on return; completion status comes from mm_workspace_check. */
int mm_values_u64_text_device_async(mm_workspace_t *ws, const void *d_text, uint64_t text_bytes, uint64_t n, int encoding,
                                    uint32_t len, int canonical, const uint32_t *d_pos, uint64_t n_pos, uint64_t *d_values);
int mm_values_u128_text_device_async(mm_workspace_t *ws, const void *d_text, uint64_t text_bytes, uint64_t n, int encoding,
                                     uint32_t len, int canonical, const uint32_t *d_pos, uint64_t n_pos, uint64_t *d_values);
/* The same from HOST memory: one upload, one launch, one download (text_bytes = n). */
int mm_values_u64_text_host(mm_workspace_t *ws, const uint8_t *text, uint64_t n, int encoding, uint32_t len, int canonical,
                            const uint32_t *pos, uint64_t n_pos, uint64_t *values);
int mm_values_u128_text_host(mm_workspace_t *ws, const uint8_t *text, uint64_t n, int encoding, uint32_t len, int canonical,
                             const uint32_t *pos, uint64_t n_pos, uint64_t *values);
/* EVERY record of a text batch in one launch: the contract of mm_values_u64_reads_device_async, on what
 * mm_run_text_batch_device_async takes and writes - what a loop over Builder::run (src/lib.rs:378) and Output::values_* per
 * record computes.  Record r is bytes [d_starts[r], d_starts[r + 1]); value i belongs to the record r with
 * d_out_offsets[r] <= i < d_out_offsets[r + 1] (empty records are skipped) and is the k-mer at byte d_starts[r] + d_pos[i].
 * The TRUE count is d_out_offsets[n_records], read on the device: nothing at or past it, or past n_pos_max, is written, so
 * a text batch run followed by its values queues on one stream with no host wait.  n_chars >= 2^32 or n_records >= 2^31:
 * MM_ERR_LEN_TOO_LARGE; n_chars > text_bytes: MM_ERR_CAPACITY.  No byte outside [d_text, d_text + text_bytes) is loaded
 * whatever d_pos, d_starts and d_out_offsets hold; a position whose k-mer runs past its record but stays inside the buffer
 * gives whatever the bytes hold (unspecified).  Otherwise as the single-text call. */
int mm_values_u64_text_batch_device_async(mm_workspace_t *ws, const void *d_text, uint64_t text_bytes, uint64_t n_records,
                                          const uint64_t *d_starts /* [n_records + 1] */, uint64_t n_chars, int encoding,
                                          uint32_t len, int canonical, const uint32_t *d_pos,
                                          const uint64_t *d_out_offsets /* [n_records + 1] */, uint64_t n_pos_max,
                                          uint64_t *d_values);
int mm_values_u128_text_batch_device_async(mm_workspace_t *ws, const void *d_text, uint64_t text_bytes, uint64_t n_records,
                                           const uint64_t *d_starts /* [n_records + 1] */, uint64_t n_chars, int encoding,
                                           uint32_t len, int canonical, const uint32_t *d_pos,
                                           const uint64_t *d_out_offsets /* [n_records + 1] */, uint64_t n_pos_max,
                                           uint64_t *d_values);
/* The values of a counts run (mm_run_text_batch_counts_device_async; Output::values_* per record, src/lib.rs:584-629):
 * max_chars / max_records / d_starts / d_counts as that call took them, d_pos / d_out_offsets as it wrote them.  The number
 * of records - for the record search and for the true count d_out_offsets[n_records] - is d_counts[1], read on the device,
 * and both counts are held against the bounds there: beyond them (the state the run refuses), or with no record, nothing
 * is written.  max_records == 0 or n_pos_max == 0 returns MM_OK with nothing launched.  Bounds, encodings and the loads'
 * limits as the call above and mm_values_u64_text_batch_device_async. */
int mm_values_u64_text_batch_counts_device_async(mm_workspace_t *ws, const void *d_text, uint64_t text_bytes,
                                                 uint64_t max_chars, uint64_t max_records,
                                                 const uint64_t *d_starts /* [max_records + 1] */,
                                                 const uint64_t *d_counts /* [2] */, int encoding, uint32_t len,
                                                 int canonical, const uint32_t *d_pos,
                                                 const uint64_t *d_out_offsets /* [max_records + 1] */, uint64_t n_pos_max,
                                                 uint64_t *d_values);
int mm_values_u128_text_batch_counts_device_async(mm_workspace_t *ws, const void *d_text, uint64_t text_bytes,
                                                  uint64_t max_chars, uint64_t max_records,
                                                  const uint64_t *d_starts /* [max_records + 1] */,
                                                  const uint64_t *d_counts /* [2] */, int encoding, uint32_t len,
                                                  int canonical, const uint32_t *d_pos,
                                                  const uint64_t *d_out_offsets /* [max_records + 1] */, uint64_t n_pos_max,
                                                  uint64_t *d_values);
/* The same from HOST memory (the text is bytes 0 .. starts[n_records], the count offsets[n_records]).  Starts or offsets
 * that decrease return MM_ERR_UNSORTED before anything is touched. */
int mm_values_u64_text_batch_host(mm_workspace_t *ws, const uint8_t *text, uint64_t n_records,
                                  const uint64_t *starts /* [n_records + 1] */, int encoding, uint32_t len, int canonical,
                                  const uint32_t *pos, const uint64_t *offsets /* [n_records + 1] */, uint64_t *values);
int mm_values_u128_text_batch_host(mm_workspace_t *ws, const uint8_t *text, uint64_t n_records,
                                   const uint64_t *starts /* [n_records + 1] */, int encoding, uint32_t len, int canonical,
                                   const uint32_t *pos, const uint64_t *offsets /* [n_records + 1] */, uint64_t *values);
/* Diagnostics of the text values kernels (Output::values_*, src/lib.rs:584-629; no device needed).
 * mm_values_text_lds_stage: the offsets a workgroup of the batch kernels stages in LDS; a workgroup whose values span more
 * records searches global memory instead.  mm_debug_values_text: the values at the ABSOLUTE positions abs_pos[0 .. n) of a
 * HOST buffer, by the very functions the kernels call for one value - the gather from whole dwords and edge bytes, the
 * 2-bit compression, the assembly and the canonical step; out holds n words (want_u128: 2n, {lo, hi}).  The refusals of
 * the device calls for encoding, canonical and len. */
uint32_t mm_values_text_lds_stage(void);
int mm_debug_values_text(const uint8_t *text, uint64_t text_bytes, int encoding, uint32_t len, int canonical, int want_u128,
                         const uint64_t *abs_pos, uint64_t n, uint64_t *out);

/* Page-locked host memory for the host entry points.  Any host pointer works; with buffers from
 * mm_host_alloc the copies to and from the device run in both directions at once (97 GB/s aggregate
 * against 56 GB/s for pageable memory on the round-1 box), which the pipelined long-sequence path
 * of mm_run_host exploits. */
int mm_host_alloc(void **out, uint64_t bytes);
void mm_host_free(void *p);

/* ------------------------------------------------------------------ batch */

/* Many independent sequences (contigs) with one plan: what the reference does by calling
 * Builder::run once per sequence (bench/src/bin/paper.rs:410-431).  Sequence s lives at
 * d_packed[s] (device pointers, host array).  Positions are sequence-local and are written back
 * to back into d_out_pos; out_offsets[s] .. out_offsets[s+1] (host array of n_seqs+1 entries)
 * delimit sequence s.  With a fused kernel for the plan the whole batch is ONE launch (every tile
 * looks its sequence up in a device table), so thousands of contigs cost no more launches than one
 * chromosome; other plans take one launch per sequence on the workspace stream. */
int mm_run_batch_device(const mm_plan_t *plan, mm_workspace_t *ws, uint64_t n_seqs,
                        const void *const *d_packed, const uint64_t *packed_bytes,
                        const uint64_t *base_offsets, const uint64_t *n_bases,
                        uint32_t *d_out_pos, uint32_t *d_out_sk, uint64_t capacity,
                        uint64_t *out_offsets);

/* Batched short reads (the read-mapping / k-mer-counting shape: millions of 100-300 bp reads, each
 * an independent Builder::run, src/lib.rs:378): read r is the bases
 * [base_offset + r * read_stride, + len_r) of one packed device buffer, len_r = d_read_lens[r]
 * (<= read_len) or read_len when d_read_lens is NULL.  Positions are read-local and written back
 * to back; d_out_offsets (device, n_reads + 1 entries) delimits the reads.  Plans run as ONE launch
 * with one lane per read (prebuilt kernels for minimizers at the common window sizes, kernels
 * specialised at first use for syncmers, super-k-mer indices and other w <= 128); only reads too
 * long for a lane's LDS list or w > 128 take one launch per read - same results. */
int mm_run_reads_device_async(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed,
                              uint64_t packed_bytes, uint64_t base_offset, uint64_t n_reads,
                              uint32_t read_stride, uint32_t read_len, const uint32_t *d_read_lens,
                              uint32_t *d_out_pos, uint64_t capacity, uint64_t *d_out_offsets,
                              uint64_t *d_count);
int mm_run_reads_device(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed,
                        uint64_t packed_bytes, uint64_t base_offset, uint64_t n_reads,
                        uint32_t read_stride, uint32_t read_len, const uint32_t *d_read_lens,
                        uint32_t *d_out_pos, uint64_t capacity, uint64_t *d_out_offsets,
                        uint64_t *out_count);

/* --------------------------------------------------------------- PackedNSeq */

/* Builder::run_skip_ambiguous_windows (src/lib.rs:451-496) on canonical_minimizers /
 * canonical_closed_syncmers / canonical_open_syncmers plans
 * (canonical_minimizers_skip_ambiguous_windows, src/minimizers.rs:169-214): a window with an
 * ambiguous base among its l = k+w-1 bases yields SKIPPED = u32::MAX-1 (src/minimizers.rs:18),
 * which the collectors then drop (collect_and_dedup_into::<true>, src/collect.rs:128-285 with
 * SKIP_MAX; src/syncmers.rs:113-120,154-164).  A PackedNSeq crosses the ABI as two arrays: the
 * PackedSeq bytes (2-bit codes; an ambiguous character carries the lossy code (c>>1)&3) and the
 * ambiguity bits, base i at bit (amb_offset + i) % 8 of byte (amb_offset + i) / 8 (packed-seq 5.0.0
 * BitSeq, not in the reference tree: layout inferred).  Non-canonical plans return
 * MM_ERR_HASHER_NOT_CANONICAL (assert src/minimizers.rs:176); there is no super-k-mer flavour. */
int mm_run_skip_ambiguous_device_async(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed,
                                       uint64_t packed_bytes, uint64_t base_offset, const void *d_amb,
                                       uint64_t amb_bytes, uint64_t amb_offset, uint64_t n_bases,
                                       uint64_t win_begin, uint64_t win_end, uint32_t *d_out_pos,
                                       uint64_t capacity, uint64_t *d_count);
int mm_run_skip_ambiguous_device(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed,
                                 uint64_t packed_bytes, uint64_t base_offset, const void *d_amb,
                                 uint64_t amb_bytes, uint64_t amb_offset, uint64_t n_bases,
                                 uint64_t win_begin, uint64_t win_end, uint32_t *d_out_pos,
                                 uint64_t capacity, uint64_t *out_count);
int mm_run_skip_ambiguous_host(const mm_plan_t *plan, mm_workspace_t *ws, const uint8_t *packed,
                               uint64_t base_offset, const uint8_t *amb, uint64_t amb_offset,
                               uint64_t n_bases, uint32_t *out_pos, uint64_t capacity,
                               uint64_t *out_count);
/* PackedNSeqVec::from_ascii (call site src/test.rs:436) then the run, from a host ASCII buffer. */
int mm_run_skip_ambiguous_host_ascii(const mm_plan_t *plan, mm_workspace_t *ws, const uint8_t *ascii,
                                     uint64_t n_bases, uint32_t *out_pos, uint64_t capacity,
                                     uint64_t *out_count);
/* The same with super-k-mer indices (Builder::super_kmers + run per read, src/lib.rs:341,545-576):
 * d_out_sk[j] = read-local index of the first window that selected d_out_pos[j].  Minimizer plans
 * only (MM_ERR_BAD_MODE otherwise, like src/lib.rs:339). */
int mm_run_reads_superkmers_device_async(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed,
                                         uint64_t packed_bytes, uint64_t base_offset, uint64_t n_reads,
                                         uint32_t read_stride, uint32_t read_len,
                                         const uint32_t *d_read_lens, uint32_t *d_out_pos,
                                         uint32_t *d_out_sk, uint64_t capacity, uint64_t *d_out_offsets,
                                         uint64_t *d_count);
int mm_run_reads_superkmers_device(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed,
                                   uint64_t packed_bytes, uint64_t base_offset, uint64_t n_reads,
                                   uint32_t read_stride, uint32_t read_len, const uint32_t *d_read_lens,
                                   uint32_t *d_out_pos, uint32_t *d_out_sk, uint64_t capacity,
                                   uint64_t *d_out_offsets, uint64_t *out_count);

/* Batched short reads with ambiguity bits (same layout rules as mm_run_reads_device; read r's
 * ambiguity bits start at bit amb_offset + r * read_stride). */
int mm_run_reads_skip_ambiguous_device_async(const mm_plan_t *plan, mm_workspace_t *ws,
                                             const void *d_packed, uint64_t packed_bytes,
                                             uint64_t base_offset, const void *d_amb, uint64_t amb_bytes,
                                             uint64_t amb_offset, uint64_t n_reads, uint32_t read_stride,
                                             uint32_t read_len, const uint32_t *d_read_lens,
                                             uint32_t *d_out_pos, uint64_t capacity,
                                             uint64_t *d_out_offsets, uint64_t *d_count);
int mm_run_reads_skip_ambiguous_device(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed,
                                       uint64_t packed_bytes, uint64_t base_offset, const void *d_amb,
                                       uint64_t amb_bytes, uint64_t amb_offset, uint64_t n_reads,
                                       uint32_t read_stride, uint32_t read_len,
                                       const uint32_t *d_read_lens, uint32_t *d_out_pos,
                                       uint64_t capacity, uint64_t *d_out_offsets, uint64_t *out_count);

/* ------------------------------------------------------------------ input */

/* PackedSeqVec::from_ascii on the device: out byte i/4 |= ((c>>1)&3) << 2(i%4). */
int mm_pack_ascii_device_async(mm_workspace_t *ws, const uint8_t *d_ascii, uint64_t n_bases,
                               uint8_t *d_packed /* ceil(n/4) bytes */);
/* PackedNSeqVec::from_ascii on the device: the packed bytes as above plus one ambiguity bit per
 * base (set for every character that is not ACGT / acgt), d_amb = ceil(n/8) bytes. */
int mm_pack_ascii_n_device_async(mm_workspace_t *ws, const uint8_t *d_ascii, uint64_t n_bases,
                                 uint8_t *d_packed /* ceil(n/4) bytes */, uint8_t *d_amb);
/* FASTA text -> PackedSeq records on the device: what the reference's loader does on the CPU with
 * needletail::parse_fastx_file + PackedSeqVec::from_ascii per record (bench/src/lib.rs:51-82).  A record
 * starts with '>' at the start of a line, its header runs to the end of that line, its sequence is every
 * following line up to the next header with '\n' and '\r' removed (bytes before the first header are
 * ignored); every sequence byte packs as (c >> 1) & 3.  ALL records go back to back into d_packed (4-byte
 * aligned, packed_capacity_bytes a multiple of 4; n_bytes / 4 + 8 always suffices): record r = bases
 * [d_rec_base[r], d_rec_base[r + 1]) of it - pass d_packed + base / 4 with base_offset = base % 4 to
 * mm_run_batch_device.  d_rec_text_pos[r] (optional) = byte offset of the record's '>' in the text (the
 * caller slices the header from there).  d_counts[0] = bases, d_counts[1] = records found; records past
 * max_records are counted but not tabulated.  The text must be shorter than 2^32 bytes.  Two passes over the text
 * (mm_fasta2.hip: every 16 KB chunk's effect on the header / record state as a composable function, then the packing);
 * nothing in them depends on line lengths or on the order workgroups start in, so the call has no failure mode of its
 * own.  (MM_FASTA_KERNEL=lines selects the one-pass kernel of rounds 3-4, which gives up on texts whose lines are
 * shorter than 16 bytes on average and on a look-back time-out - the synchronous call below then repeats the text with
 * the three-pass kernels, an asynchronous caller gets MM_ERR_ORDER from mm_workspace_check(); MM_FASTA_KERNEL=three
 * takes those from the start.  Both are kept as cross-checks.) */
int mm_fasta_pack_device_async(mm_workspace_t *ws, const uint8_t *d_text, uint64_t n_bytes,
                               uint8_t *d_packed, uint64_t packed_capacity_bytes,
                               uint64_t *d_rec_base /* [max_records + 1] */,
                               uint64_t *d_rec_text_pos /* [max_records] or NULL */, uint64_t max_records,
                               uint64_t *d_counts /* [2] */);
/* The same, synchronous: out_counts[0..1] receive the counts; MM_ERR_CAPACITY when the bases did not fit
 * d_packed or the records did not fit the table (the counts say what is needed: out_counts[0] against
 * 4 * packed_capacity_bytes, out_counts[1] against max_records).  A text whose first non-blank byte is '@'
 * is FASTQ, which the reference's loader reads through the same call (needletail::parse_fastx_file): since
 * round 4 this entry point looks at that byte and packs FASTQ with mm_fastq_pack_device_async (same outputs).
 * The asynchronous FASTA entry point above does not look and would pack no record from a FASTQ text. */
int mm_fasta_pack_device(mm_workspace_t *ws, const uint8_t *d_text, uint64_t n_bytes, uint8_t *d_packed,
                         uint64_t packed_capacity_bytes, uint64_t *d_rec_base, uint64_t *d_rec_text_pos,
                         uint64_t max_records, uint64_t *d_counts, uint64_t *out_counts /* [2] */);
/* Reads packed BACK TO BACK (round 4): read r = bases [d_read_starts[r], d_read_starts[r + 1]) of one packed buffer -
 * the layout mm_fastq_pack_device_async / mm_fasta_pack_device write (d_rec_base), so millions of reads of ANY
 * lengths run in ONE launch of the reads-mode kernel (mm_run_batch_device gives every sequence tiles of its own,
 * which is right for contigs and wasteful for reads).  d_read_starts: n_reads + 1 device entries; total_bases =
 * d_read_starts[n_reads] (the packer's count of bases); max_read_len: no read is longer (a longer one is cut to it,
 * like a d_read_lens entry above read_len).  Positions are read-local, d_out_offsets[r] .. [r + 1] delimit read r's;
 * d_out_sk (or NULL): super-k-mer indices.  Builder::run per read, src/lib.rs:378. */
int mm_run_packed_reads_device_async(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed,
                                     uint64_t packed_bytes, uint64_t base_offset, uint64_t n_reads,
                                     const uint64_t *d_read_starts /* [n_reads + 1] */, uint64_t total_bases,
                                     uint32_t max_read_len, uint32_t *d_out_pos, uint32_t *d_out_sk /* or NULL */,
                                     uint64_t capacity, uint64_t *d_out_offsets /* [n_reads + 1] */, uint64_t *d_count);
int mm_run_packed_reads_device(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed,
                               uint64_t packed_bytes, uint64_t base_offset, uint64_t n_reads,
                               const uint64_t *d_read_starts, uint64_t total_bases, uint32_t max_read_len,
                               uint32_t *d_out_pos, uint32_t *d_out_sk, uint64_t capacity, uint64_t *d_out_offsets,
                               uint64_t *out_count);
/* The same from HOST memory in one call: n_reads reads packed back to back in `packed` (read r = bases
 * [read_starts[r], read_starts[r + 1]), starts on the host, non-decreasing), one upload, ONE launch, one download.
 * What a caller that looped Builder::run over its reads does instead: a synchronous call costs about 28 us whatever
 * the length, so a per-read loop runs 10-100 x slower than the reference's CPU on 150-base reads, and this call does
 * millions of them at PCIe speed.  out_offsets[r] .. [r + 1] delimit read r's (read-local) positions. */
int mm_run_packed_reads_host(const mm_plan_t *plan, mm_workspace_t *ws, const uint8_t *packed, uint64_t n_reads,
                             const uint64_t *read_starts /* [n_reads + 1] */, uint32_t max_read_len, uint32_t *out_pos,
                             uint32_t *out_sk /* or NULL */, uint64_t capacity, uint64_t *out_offsets /* [n_reads + 1] */,
                             uint64_t *out_count);
/* FASTQ text -> packed records (round 4; mm_fastq.hip): four-line records ('@' name, sequence, '+', qualities;
 * "\r\n" or '\n', a last line without '\n', blank lines after the last record); the sequence of every record is
 * packed like a FASTA record's, same output layout: record r = bases [d_rec_base[r], d_rec_base[r + 1]),
 * d_rec_text_pos[r] = byte offset of its '@', d_counts = {bases, records}.  Reads of one length go straight into
 * mm_run_reads_device (read_stride = read_len), any lengths into mm_run_batch_device.  needletail is not in the
 * reference tree: parity unpinned like the FASTA packer's; no validation of '+' lines or quality lengths.
 * The text has to START with the first record's '@' (a line's role is the number of newlines in front of it mod 4);
 * mm_fasta_pack_device cuts blank bytes in front of it off before it calls this and keeps the text positions absolute. */
int mm_fastq_pack_device_async(mm_workspace_t *ws, const uint8_t *d_text, uint64_t n_bytes,
                               uint8_t *d_packed, uint64_t packed_capacity_bytes,
                               uint64_t *d_rec_base /* [max_records + 1] */,
                               uint64_t *d_rec_text_pos /* [max_records] or NULL */, uint64_t max_records,
                               uint64_t *d_counts /* [2] */);
/* FASTA / FASTQ text with N: the packers above, which ALSO write the ambiguity bits of a PackedNSeq, and the
 * skip-ambiguous run over the records they write - file -> minimizers with Builder::run_skip_ambiguous_windows per
 * record (src/lib.rs:451-496, src/minimizers.rs:169-214) and no parsing on the CPU.
 *
 * d_packed, d_rec_base, d_rec_text_pos and d_counts receive exactly what the plain packer writes for the same text.
 * d_amb receives one bit per output base in the numbering of d_packed: base i is bit i % 8 of byte i / 8, record r
 * owns bits [d_rec_base[r], d_rec_base[r + 1]).  A bit is set for every sequence byte whose upper-cased value
 * (c & 0xDF) is not one of A C G T - the rule of mm_pack_ascii_n_device_async; line ends, header and quality bytes
 * are not bases and give no bit.  d_amb: not NULL and 4-byte aligned (MM_ERR_NULL otherwise, like d_packed);
 * amb_capacity_bytes: a non-zero multiple of 4 (MM_ERR_CAPACITY otherwise); n_bytes / 8 + 8 rounded up to a multiple
 * of 4 always suffices.  The first min(amb_capacity_bytes, that) bytes are cleared, nothing is written past
 * amb_capacity_bytes.  Always the two-pass kernels (MM_FASTA_KERNEL does not apply).  The asynchronous FASTQ entry
 * wants the text to start with its first '@', like mm_fastq_pack_device_async. */
int mm_fasta_pack_n_device_async(mm_workspace_t *ws, const uint8_t *d_text, uint64_t n_bytes,
                                 uint8_t *d_packed, uint64_t packed_capacity_bytes,
                                 uint8_t *d_amb, uint64_t amb_capacity_bytes,
                                 uint64_t *d_rec_base /* [max_records + 1] */,
                                 uint64_t *d_rec_text_pos /* [max_records] or NULL */, uint64_t max_records,
                                 uint64_t *d_counts /* [2] */);
int mm_fastq_pack_n_device_async(mm_workspace_t *ws, const uint8_t *d_text, uint64_t n_bytes,
                                 uint8_t *d_packed, uint64_t packed_capacity_bytes,
                                 uint8_t *d_amb, uint64_t amb_capacity_bytes,
                                 uint64_t *d_rec_base /* [max_records + 1] */,
                                 uint64_t *d_rec_text_pos /* [max_records] or NULL */, uint64_t max_records,
                                 uint64_t *d_counts /* [2] */);
/* Synchronous; FASTQ is told from FASTA by the first non-blank byte, as mm_fasta_pack_device does.  MM_ERR_CAPACITY
 * also when the bases did not fit d_amb (out_counts[0] against 8 * amb_capacity_bytes). */
int mm_fasta_pack_n_device(mm_workspace_t *ws, const uint8_t *d_text, uint64_t n_bytes, uint8_t *d_packed,
                           uint64_t packed_capacity_bytes, uint8_t *d_amb, uint64_t amb_capacity_bytes,
                           uint64_t *d_rec_base, uint64_t *d_rec_text_pos, uint64_t max_records,
                           uint64_t *d_counts, uint64_t *out_counts /* [2] */);
/* Builder::run_skip_ambiguous_windows (src/lib.rs:451-496; the skipping collect src/minimizers.rs:169-214) per record
 * of a back-to-back buffer: mm_run_packed_reads_device with the ambiguity bits of the same bases (base j of the
 * buffer = bit amb_offset + j of d_amb).  One launch - one lane per read or the lane table - with the window
 * ambiguity prepared once over the whole span: a window that lies inside a record covers that record's bases only,
 * so a neighbour's N never reaches it.  Canonical minimizer / closed-syncmer / open-syncmer plans
 * (MM_ERR_HASHER_NOT_CANONICAL for a forward plan, MM_ERR_BAD_MODE for a text plan); no super-k-mer flavour, as the
 * reference has none.  Positions are record-local, d_out_offsets[r] .. [r + 1] delimit record r's. */
int mm_run_packed_reads_skip_ambiguous_device_async(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed,
                                                    uint64_t packed_bytes, uint64_t base_offset, const void *d_amb,
                                                    uint64_t amb_bytes, uint64_t amb_offset, uint64_t n_reads,
                                                    const uint64_t *d_read_starts /* [n_reads + 1] */,
                                                    uint64_t total_bases, uint32_t max_read_len, uint32_t *d_out_pos,
                                                    uint64_t capacity, uint64_t *d_out_offsets /* [n_reads + 1] */,
                                                    uint64_t *d_count);
int mm_run_packed_reads_skip_ambiguous_device(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed,
                                              uint64_t packed_bytes, uint64_t base_offset, const void *d_amb,
                                              uint64_t amb_bytes, uint64_t amb_offset, uint64_t n_reads,
                                              const uint64_t *d_read_starts, uint64_t total_bases,
                                              uint32_t max_read_len, uint32_t *d_out_pos, uint64_t capacity,
                                              uint64_t *d_out_offsets, uint64_t *out_count);
/* The same from HOST memory in one call, like mm_run_packed_reads_host: `packed` and `amb` hold the reads back to back
 * from base 0 (ceil(total / 4) and ceil(total / 8) bytes, total = read_starts[n_reads]). */
int mm_run_packed_reads_skip_ambiguous_host(const mm_plan_t *plan, mm_workspace_t *ws, const uint8_t *packed,
                                            const uint8_t *amb, uint64_t n_reads,
                                            const uint64_t *read_starts /* [n_reads + 1] */, uint32_t max_read_len,
                                            uint32_t *out_pos, uint64_t capacity,
                                            uint64_t *out_offsets /* [n_reads + 1] */, uint64_t *out_count);
/* The packed reads run with its two counts taken from the DEVICE: d_counts has the packers' layout (d_counts[0] = bases,
 * d_counts[1] = records, as mm_fastq_pack_device_async / mm_fasta_pack_device_async leave it) and is read when the kernels
 * run, so a packer, this call and mm_values_*_reads_device_async (with n_reads = max_records) queue on one stream and the
 * caller waits once (mm_workspace_check) - FASTQ / FASTA in device memory -> records -> positions -> values with no host
 * wait in between.  It replaces reading the packer's counts back before mm_run_packed_reads_device_async.  The reference
 * has no counterpart: its loader and Builder::run are synchronous host code (bench/src/lib.rs:51-82, src/lib.rs:378).
 *  max_bases / max_records  upper bounds of the two counts, all the host knows: they size the lane table, the walk's grid
 *                         and the workspace buffers.  Behind a packer: 4 * packed_capacity_bytes (or the text length) and
 *                         the packer's max_records
 *  d_read_starts          [max_records + 1]; with (n_bases, n_records) = d_counts[0..1] at kernel time, entries past
 *                         [n_records] are never used to form an address or a length, and starts are cut to n_bases
 *  d_out_pos / d_out_sk / d_out_offsets[0 .. n_records] / d_count
 *                         bit for bit what mm_run_packed_reads_device_async writes given n_records, n_bases and
 *                         max_read_len = 0xffffffff as host arguments
 *  d_out_offsets[n_records .. max_records]
 *                         all hold the total: the tail is FILLED (reads past n_records are empty), so
 *                         mm_values_u64/u128_reads_device_async follows on the same stream with n_reads = max_records
 * The run ALWAYS takes the lane table (mm_lanes.hip): one lane per read needs max_read_len and n_reads inside the walk.  For
 * short reads of one length a caller who knows its counts keeps mm_run_packed_reads_device / mm_run_reads_device.
 * No read (n_records == 0) or no read of l = k + w - 1 bases: count 0 and every offset 0, written by the kernels.  Counts
 * BEYOND a bound (d_counts[0] > max_bases or d_counts[1] > max_records: a packer whose buffer or table was too small): the
 * run behaves as an empty batch - count 0, every offset 0, d_out_pos untouched - and mm_workspace_check returns
 * MM_ERR_CAPACITY (kernel error 7; mm_last_error() names this call).  No byte outside [d_packed, d_packed + packed_bytes)
 * is loaded whatever d_counts and d_read_starts hold.
 * Refusals before anything is queued, in this order, the same in both forms: NULL plan (MM_ERR_NULL); a text plan
 * (MM_ERR_BAD_MODE); max_bases >= 2^32 or max_records >= 2^31 (MM_ERR_LEN_TOO_LARGE); d_out_sk with syncmers
 * (MM_ERR_BAD_MODE); a forward plan in the skip-ambiguous form (MM_ERR_HASHER_NOT_CANONICAL); d_packed, d_read_starts,
 * d_counts, d_out_offsets (or d_amb) NULL (MM_ERR_NULL); base_offset + max_bases beyond 4 * packed_bytes, or amb_offset +
 * max_bases beyond 8 * amb_bytes (MM_ERR_CAPACITY); a plan without a lane-table launch - mm_workspace_force_generic, w >
 * 128, no reads-mode kernel with MM_JIT=0, MM_LANE_TABLE=0, no lane length that fits - MM_ERR_BAD_MODE, and
 * mm_last_error() points to mm_run_packed_reads_device; a NULL workspace last (MM_ERR_NULL).
 * Kernels: the four table kernels in their counts instantiation (two for max_records <= 2048), the reads-mode walk with a
 * grid for max_records + max_bases / S + 1 lanes, and an epilogue that fills the offsets' tail. */
int mm_run_packed_reads_counts_device_async(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed,
                                            uint64_t packed_bytes, uint64_t base_offset, uint64_t max_bases,
                                            uint64_t max_records, const uint64_t *d_read_starts /* [max_records + 1] */,
                                            const uint64_t *d_counts /* [2]: bases, records */, uint32_t *d_out_pos,
                                            uint32_t *d_out_sk /* or NULL */, uint64_t capacity,
                                            uint64_t *d_out_offsets /* [max_records + 1] */, uint64_t *d_count);
/* Same, then waits ONCE and returns out[0] = positions, out[1] = n_bases, out[2] = n_records (a look-back time-out repeats
 * the run, as in every synchronous form; the asynchronous form reports it as MM_ERR_ORDER from mm_workspace_check).
 * MM_ERR_CAPACITY when the positions exceeded `capacity` (out[0]: the need) or the counts exceeded the bounds (out[0] = 0,
 * out[1..2]: the true counts). */
int mm_run_packed_reads_counts_device(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed, uint64_t packed_bytes,
                                      uint64_t base_offset, uint64_t max_bases, uint64_t max_records,
                                      const uint64_t *d_read_starts, const uint64_t *d_counts, uint32_t *d_out_pos,
                                      uint32_t *d_out_sk, uint64_t capacity, uint64_t *d_out_offsets,
                                      uint64_t *out /* [3]: positions, n_bases, n_records */);
/* Builder::run_skip_ambiguous_windows per record (src/lib.rs:451-496) with the counts on the device: the counts form of
 * mm_run_packed_reads_skip_ambiguous_device_async, behind mm_fastq_pack_n_device_async / mm_fasta_pack_n_device_async on one
 * stream.  The window ambiguity is prepared over the bound span max_bases (the packers clear d_amb; a lane only reads window
 * bits inside its record).  Canonical plans, no super-k-mer indices; everything else as above. */
int mm_run_packed_reads_skip_ambiguous_counts_device_async(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed,
                                                           uint64_t packed_bytes, uint64_t base_offset, const void *d_amb,
                                                           uint64_t amb_bytes, uint64_t amb_offset, uint64_t max_bases,
                                                           uint64_t max_records,
                                                           const uint64_t *d_read_starts /* [max_records + 1] */,
                                                           const uint64_t *d_counts /* [2]: bases, records */,
                                                           uint32_t *d_out_pos, uint64_t capacity,
                                                           uint64_t *d_out_offsets /* [max_records + 1] */,
                                                           uint64_t *d_count);
int mm_run_packed_reads_skip_ambiguous_counts_device(const mm_plan_t *plan, mm_workspace_t *ws, const void *d_packed,
                                                     uint64_t packed_bytes, uint64_t base_offset, const void *d_amb,
                                                     uint64_t amb_bytes, uint64_t amb_offset, uint64_t max_bases,
                                                     uint64_t max_records, const uint64_t *d_read_starts,
                                                     const uint64_t *d_counts, uint32_t *d_out_pos, uint64_t capacity,
                                                     uint64_t *d_out_offsets,
                                                     uint64_t *out /* [3]: positions, n_bases, n_records */);
/* What the table kernels of the calls above make of counts and bounds, by the function they call themselves (no device; for
 * tests): out[0] = reads the table is built for (n_records; 0 when refused), out[1] = 1 when a count exceeds its bound
 * (refused), out[2] = the lane bound at one window per lane, max_records + max_bases + 1 (the grid of a run is sized from
 * max_records + max_bases / S + 1 at S windows per lane, never more).  The entry points' rule for the bounds:
 * MM_ERR_LEN_TOO_LARGE for max_bases >= 2^32 or max_records >= 2^31; MM_ERR_NULL. */
int mm_debug_lane_counts_view(uint64_t max_bases, uint64_t max_records, uint64_t n_bases, uint64_t n_records,
                              uint64_t out[3]);
/* ------------------------------------------------------------------ a file of any size, in chunks
 * FASTA / FASTQ text of ANY size through the device: the caller feeds host bytes in calls of any size, the stream cuts them
 * into chunks of chunk_bytes so that no record is split, and every chunk runs packer -> counts run -> values (the calls
 * above) on a slot with a stream of its own, several chunks in flight: the upload of one chunk, the kernels of another and
 * the download of a third overlap.  The reference has no counterpart beyond "the loader reads any file"
 * (needletail::parse_fastx_file, bench/src/lib.rs:51-82, record by record on the CPU, Builder::run per record,
 * src/lib.rs:378); the results per record are those of the one-shot calls on the whole file.
 *   The cut rule (csrc/mm_fastx_cut.h; every chunk but the last): FASTQ - behind the 4 * floor(N / 4)-th of the chunk's N
 *   newlines; FASTA - at the last record's '>' (with no record yet: behind the last newline).  What lies behind the cut
 *   goes in front of the next chunk, so a packer sees at most 2 * chunk_bytes bytes.
 *   mm_fastx_stream_feed    copies into the filling slot's page-locked staging buffer and launches the slot when it holds
 *                           chunk_bytes new bytes; *consumed < n_bytes only when no slot is free: call mm_fastx_stream_next
 *   mm_fastx_stream_finish  no more bytes: the part-filled slot (and the last tail) is launched as the last chunk
 *   mm_fastx_stream_next    MM_OK and the OLDEST launched batch when it is complete, when no slot is free to fill, or after
 *                           finish (then it waits); else MM_FASTX_NEED_INPUT; MM_FASTX_END once everything is drained.  A
 *                           batch's pointers are page-locked host memory, valid until the following call of
 *                           mm_fastx_stream_next or mm_fastx_stream_destroy.  With the default of 3 slots one is read by the
 *                           caller, one runs and one fills.
 * Offsets: rec_text_pos, text_begin and text_end are ABSOLUTE (first_byte + every byte consumed before) and 64-bit - the
 * 2^32 limit of the packers holds per chunk only; the batches' [text_begin, text_end) tile the fed bytes.  Everything else is
 * chunk-local: rec_base and offsets start at 0 in every batch, positions are record-local.
 * Format: MM_FASTX_AUTO decides by the first non-blank byte, as mm_fasta_pack_device does ('@' / '>', anything else:
 * MM_ERR_FORMAT); blank bytes in front of a FASTQ are passed over and counted in the offsets.  A stream with no bytes, or
 * blank ones only, gives MM_FASTX_END and no batch.
 * Errors (a failing stream stays failed: every later call returns the same code, destroy works): MM_ERR_CAPACITY for a
 * chunk that is not the last and has no cut (a record longer than chunk_bytes; FASTA chromosomes: MM_FASTX_LONG_RECORDS), for
 * more than max_records records or more than max_positions positions in a chunk - mm_last_error() names the bound and the
 * need.  A look-back time-out of a chunk's run (MM_ERR_ORDER) repeats that run, as every synchronous form does.
 * Refusals of mm_fastx_stream_create before any device is touched, in this order: NULL arguments (MM_ERR_NULL); a text plan
 * (MM_ERR_BAD_MODE); chunk_bytes outside [64, 2^31) or max_records >= 2^31 (MM_ERR_LEN_TOO_LARGE); MM_FASTX_SK with syncmers
 * or with MM_FASTX_SKIP_AMBIGUOUS (MM_ERR_BAD_MODE); a forward plan with MM_FASTX_SKIP_AMBIGUOUS
 * (MM_ERR_HASHER_NOT_CANONICAL); both values flags (MM_ERR_BAD_MODE); a value length above 32 / 64 (MM_ERR_VALUE_LEN); a plan
 * without a lane-table launch (MM_ERR_BAD_MODE, as mm_run_packed_reads_counts_device_async says); an unknown format, flag or
 * slots outside 0, 2..8 (MM_ERR_BAD_MODE); MM_FASTX_ONE_MINIMIZER with MM_FASTX_LONG_RECORDS (MM_ERR_BAD_MODE: a split
 * record's minimizer is not joined across its pieces); MM_FASTX_LONG_RECORDS with chunk_bytes < 4 * (k + w - 1)
 * (MM_ERR_CAPACITY); no device (MM_ERR_NO_DEVICE).
 * MM_FASTX_ONE_MINIMIZER (this entry only; the values 32, 64 and 128 stay refused here): behind the run and the values every
 * chunk queues, on its slot's stream, mm_one_minimizer_reads_counts_device_async - with MM_FASTX_SKIP_AMBIGUOUS
 * mm_one_minimizer_reads_skip_ambiguous_counts_device_async over the slot's ambiguity bits - with the plan's k and hasher;
 * a repeated run queues it again, the delivered records' words are downloaded with the batch, and the stream still waits
 * for the host once per chunk.  mm_fastx_stream_one_minimizer hands them out; mm_fastx_batch_t keeps its layout.
 * A stream is used by one thread at a time, like a workspace; the plan must outlive it; every entry restores the caller's
 * current device.  Memory per slot: csrc/mm_fastx_stream.hip and DESIGN.md 4.4e. */
typedef struct mm_fastx_stream mm_fastx_stream_t;
enum { MM_FASTX_AUTO = 0, MM_FASTX_FASTA = 1, MM_FASTX_FASTQ = 2 };
enum { MM_FASTX_SK = 1, MM_FASTX_SKIP_AMBIGUOUS = 2, MM_FASTX_VALUES_U64 = 4, MM_FASTX_VALUES_U128 = 8,
       MM_FASTX_LONG_RECORDS = 16, MM_FASTX_ONE_MINIMIZER = 256 };
enum { MM_FASTX_NEED_INPUT = 1, MM_FASTX_END = 2 };           /* positive: not errors */
typedef struct mm_fastx_stream_config {
    int device; int format; uint32_t flags; uint32_t slots;    /* slots: 0 = default (3), else 2..8 */
    uint64_t chunk_bytes;      /* new bytes per chunk; 64 <= chunk_bytes < 2^31 */
    uint64_t max_records;      /* per chunk */
    uint64_t max_positions;    /* per chunk; 0 = worst case (2 * chunk_bytes) */
    uint64_t first_byte;       /* absolute offset of the first byte fed (resuming / sharding a file) */
} mm_fastx_stream_config_t;
typedef struct mm_fastx_batch {
    uint64_t n_records, n_bases, n_positions;
    uint64_t text_begin, text_end;      /* absolute byte range [begin, end) of the file this batch covers */
    const uint64_t *rec_text_pos;       /* [n_records]  absolute offset of each record's '>' / '@' */
    const uint64_t *rec_base;           /* [n_records + 1] record r has rec_base[r+1] - rec_base[r] bases */
    const uint64_t *offsets;            /* [n_records + 1] into pos / sk / values, offsets[0] = 0 */
    const uint32_t *pos, *sk;           /* record-local; sk NULL without MM_FASTX_SK */
    const uint64_t *values;             /* NULL without a values flag; u128: two words per value */
} mm_fastx_batch_t;
int  mm_fastx_stream_create(mm_fastx_stream_t **out, const mm_plan_t *plan, const mm_fastx_stream_config_t *cfg);
int  mm_fastx_stream_feed(mm_fastx_stream_t *s, const uint8_t *text, uint64_t n_bytes, uint64_t *consumed);
int  mm_fastx_stream_finish(mm_fastx_stream_t *s);
int  mm_fastx_stream_next(mm_fastx_stream_t *s, mm_fastx_batch_t *out);
void mm_fastx_stream_destroy(mm_fastx_stream_t *s);
/* Of the batch last returned by mm_fastx_stream_next (valid as long as the batch is): one word per record, record-local,
 * MM_NO_MINIMIZER for a record without a (clean) k-mer.  NULL and 0 without MM_FASTX_ONE_MINIMIZER, before the first batch
 * and on a byte-text stream (mm_fastx_text_stream_extras serves that one).  MM_ERR_NULL for a NULL argument. */
int mm_fastx_stream_one_minimizer(const mm_fastx_stream_t *s, const uint32_t **one_min, uint64_t *n_records);
/* ---- The same for BYTE TEXT (protein FASTA of any size): a text plan (mm_plan_create_text) in place of the packed one; the
 * handle is the same type and mm_fastx_stream_feed / _finish / _next / _destroy serve it unchanged.  The reference reads such
 * a file record by record on the CPU too (needletail::parse_fastx_file, bench/src/lib.rs:51-82; Builder::run on &[u8],
 * src/lib.rs:378) and has no other counterpart.  Every chunk runs, on its slot's stream, the slot pipeline of the DNA stream
 * step for step: upload, the previous chunk's tail, mm_fasta_text_device_async (the sequence bytes as they stand, into a
 * buffer of 2 * chunk_bytes), the trim step with the FASTA rule, mm_run_text_batch_counts_device_async with max_chars = the
 * chunk's text length, mm_values_*_text_batch_counts_device_async with `values_encoding`, and with
 * MM_FASTX_TEXT_ONE_MINIMIZER mm_one_minimizer_text_batch_counts_device_async with the plan's k and hasher (one_minimizer,
 * src/minimizers.rs:22-28, per record); one mm_workspace_check judges a chunk, a look-back time-out repeats run, values and
 * one minimizer.  Exactly the filled parts are downloaded.
 * The batch: mm_fastx_batch_t with n_bases = characters and rec_base = the records' starts in the chunk's byte sequence;
 * mm_fastx_text_stream_extras hands out, for the batch last returned, one_min ([n_records], record-local, MM_NO_MINIMIZER for
 * a record shorter than k; NULL without the flag) and seq (rec_base[n_records] bytes; NULL without MM_FASTX_TEXT_SEQ).
 * Offsets as above: rec_text_pos, text_begin, text_end absolute and 64-bit, everything else chunk-local.
 * Format: FASTA only (FASTQ to byte records is not provided): MM_FASTX_FASTQ is MM_ERR_FORMAT at create; with MM_FASTX_AUTO
 * a first non-blank byte '@' - or any other but '>' - is MM_ERR_FORMAT at feed.
 * Flags: MM_FASTX_SK, MM_FASTX_VALUES_U64, MM_FASTX_VALUES_U128 as above; MM_FASTX_TEXT_ONE_MINIMIZER and MM_FASTX_TEXT_SEQ
 * for this entry only; MM_FASTX_SKIP_AMBIGUOUS and MM_FASTX_LONG_RECORDS are refused (byte text has neither).
 * Refusals of mm_fastx_text_stream_create before any device is touched, in this order: NULL arguments (MM_ERR_NULL); a plan
 * that is not a text plan (MM_ERR_BAD_MODE); chunk_bytes outside [64, 2^31) or max_records >= 2^31 (MM_ERR_LEN_TOO_LARGE);
 * MM_FASTX_SK with syncmers (MM_ERR_BAD_MODE); MM_FASTX_SKIP_AMBIGUOUS or MM_FASTX_LONG_RECORDS (MM_ERR_BAD_MODE); both values
 * flags (MM_ERR_BAD_MODE); an unknown values_encoding (MM_ERR_BAD_MODE); with a values flag MM_TEXT_VALUES_BYTES and a
 * canonical hasher (MM_ERR_BAD_MODE), then a value length beyond the encoding's limit - 8 / 16 for BYTES, 32 / 64 for DNA
 * (MM_ERR_VALUE_LEN); a plan the fused text kernel does not take, w > 128 or k > 1024 (MM_ERR_BAD_MODE, mm_last_error() as
 * mm_run_text_batch_counts_device_async sets it); format MM_FASTX_FASTQ (MM_ERR_FORMAT); an unknown format, flag or slots
 * outside 0, 2..8 (MM_ERR_BAD_MODE); no device (MM_ERR_NO_DEVICE).
 * Errors while streaming as above (the stream stays failed): MM_ERR_CAPACITY for a record longer than a chunk, more than
 * max_records records or more than max_positions positions in a chunk.  Memory per slot: DESIGN.md 4.4e. */
enum { MM_FASTX_TEXT_ONE_MINIMIZER = 32, MM_FASTX_TEXT_SEQ = 64 };
typedef struct mm_fastx_text_stream_config {
    int device; int format; uint32_t flags; uint32_t slots;    /* as mm_fastx_stream_config_t */
    uint64_t chunk_bytes, max_records, max_positions, first_byte;
    int values_encoding;       /* MM_TEXT_VALUES_BYTES / MM_TEXT_VALUES_DNA */
} mm_fastx_text_stream_config_t;
typedef struct mm_fastx_text_extras {
    const uint32_t *one_min;   /* [n_records] record-local, MM_NO_MINIMIZER: shorter than k; NULL without the flag */
    const uint8_t *seq;        /* [rec_base[n_records]] the records' bytes back to back; NULL without the flag */
} mm_fastx_text_extras_t;
int mm_fastx_text_stream_create(mm_fastx_stream_t **out, const mm_plan_t *text_plan, const mm_fastx_text_stream_config_t *cfg);
/* Of the batch last returned by mm_fastx_stream_next (valid as long as the batch is; NULLs before the first batch and for a
 * stream of mm_fastx_stream_create). */
int mm_fastx_text_stream_extras(const mm_fastx_stream_t *s, mm_fastx_text_extras_t *out);
/* The cut rule on a text in HOST memory, by the function the trim kernel calls itself (csrc/mm_fastx_cut.h; no device, like
 * mm_debug_lane_counts_view): format MM_FASTX_FASTA / MM_FASTX_FASTQ (MM_ERR_BAD_MODE otherwise), last != 0 keeps everything;
 * out = {cut, kept records, dropped records}. */
int mm_debug_fastx_cut(const uint8_t *text, uint64_t n, int format, int last, uint64_t out[3]);
/* ---- FASTA records longer than a chunk: MM_FASTX_LONG_RECORDS (genome FASTA: chromosomes of any length below 2^32 bases)
 * Opt-in; without the flag every batch and every error is as described above, and the flag acts on FASTA text only (a FASTQ
 * stream, explicit or found by MM_FASTX_AUTO, behaves as without it).  With it, a chunk in which the FASTA rule finds no
 * cut is no longer an error when the chunk is ONE record from its first byte on and that record's header line is complete:
 * the whole chunk is delivered as a PIECE of an OPEN record, and the next chunk's device text begins with a synthetic header
 * line ">\n" followed by the piece's last l - 1 sequence bytes (l = k + w - 1; text[T, n), T from the trim step) - the
 * packers, the run and the values calls see an ordinary FASTA whose record 0 begins with the l - 1 overlap bases.  A seam
 * epilogue makes the result exact: record 0's positions (and super-k-mer indices, which are window indices) get
 * first_base added on the device, behind the values; for minimizers the piece's first position is dropped, with its
 * index and value, when it equals the last position the record emitted before (a lane's first window always emits; the
 * rule by which the reference joins lanes, src/collect.rs:265-271, and mm_run_device_async joins window ranges) - so
 *   positions, indices and values of one record are the concatenation of its pieces' slices, in order, and equal what
 *   the one-shot calls give for the whole record.
 * What a batch says about pieces (valid for the batch last returned by mm_fastx_stream_next; all zeros without the flag,
 * for FASTQ, and for batches without a piece):
 *   first_continues  record 0 continues the previous batch's last record: rec_text_pos[0] is the absolute offset of the
 *                    record's real '>' (the same in every piece); rec_base counts what the packer wrote, the first_overlap
 *                    repeated bases included; pos / sk of record 0 are record-global (piece-local + first_base)
 *   last_open        the last record goes on in the next batch (such a batch holds that one record only)
 *   first_base       the record-global index of record 0's first packed base: the record's bases delivered before, minus
 *                    first_overlap
 *   first_overlap    how many of record 0's bases repeat the end of the previous piece: l - 1, or all it had
 * so a record has sum(piece bases) - sum(first_overlap) bases.  text_begin / text_end still tile the fed bytes (a piece
 * covers exactly its chunk's new bytes), offsets still start at 0 and n_positions counts what is delivered.
 * Errors with the flag, the stream stays failed: MM_ERR_CAPACITY for a chunk that begins with a header line that does not
 * end inside it ("a record longer than chunk_bytes", as without the flag), for a piece that brings no new base of its record
 * ("cannot advance": a chunk of line ends), for an overlap text longer than chunk_bytes; MM_ERR_LEN_TOO_LARGE for a record
 * that reaches 2^32 bases.  Still out: FASTQ records longer than a chunk, records of 2^32 bases or more, several devices,
 * plain (non-BGZF) gzip.  A sequence line that begins with '>' is a header line, as everywhere; a '>' inside a sequence line is a base the
 * packers map like any other letter, but must not be the first of the l - 1 overlap bytes' line (it would read as a header).
 * Memory: the carry area grows by 16 bytes (2 are used); a packer sees at most 2 * chunk_bytes + 2 bytes. */
typedef struct mm_fastx_pieces {
    uint32_t first_continues;  /* record 0 continues the previous batch's last record */
    uint32_t last_open;        /* the last record goes on in the next batch */
    uint64_t first_base;       /* record-global index of record 0's first packed base (0 if !first_continues) */
    uint64_t first_overlap;    /* how many of record 0's bases repeat the previous piece (l-1 or fewer; else 0) */
} mm_fastx_pieces_t;
int mm_fastx_stream_pieces(const mm_fastx_stream_t *s, mm_fastx_pieces_t *out);
/* The split rule on a FASTA text in HOST memory (csrc/mm_fastx_cut.h, the function the trim kernel calls; no device):
 * l = k + w - 1; out = {cut, T, open, overlap} - open = 1: the chunk is a piece (cut = n), T the offset of its (l - 1)-th
 * sequence byte from the end ('\n' and '\r' are no sequence bytes), never inside the header line (fewer than l - 1: the
 * first sequence byte, n when there is none), overlap the sequence bytes in text[T, n); open = 0: cut is
 * mm_debug_fastx_cut's and T = overlap = 0. */
int mm_debug_fastx_split(const uint8_t *text, uint64_t n, uint32_t l, int last, uint64_t out[4]);
/* ------------------------------------------------------------------ BGZF-compressed input, inflated on the device
 * BGZF (bgzip, htslib: most .fastq.gz / .fa.gz that pipelines write) is a series of independent gzip members of at most
 * 64 KiB of text each; every member says its compressed size in its header (extra subfield BC: BSIZE) and its text size in
 * its trailer (ISIZE).  The host lays out the output from the headers alone, the device inflates the blocks side by side,
 * one wavefront per block (csrc/mm_bgzf.hip; the decoder, RFC 1951 with stored, fixed and dynamic blocks, is
 * csrc/mm_inflate.h, the same code on host and device).  The reference reads compressed files through its loader on the
 * CPU (needletail::parse_fastx_file, bench/src/lib.rs:51-82) and has no other counterpart.
 * The inflate accepts a block when its deflate stream is well formed, ends with its final block's end-of-block code and
 * gives exactly ISIZE bytes; payload bytes behind the final block are ignored.  CRC32 IS VERIFIED ON REQUEST, as zlib,
 * htslib and the reference's loader verify it: a kernel of its own (csrc/mm_crc32.hip, one workgroup of 256 threads per
 * block; the arithmetic is csrc/mm_crc32.h, the same code on host and device) computes the CRC32 of every block's text
 * where the inflate has written it and compares it with the block's gzip trailer - mm_bgzf_crc32_device_async,
 * mm_bgzf_inflate_verify_host and, for the stream, the flag MM_FASTX_BGZF_CRC below.  Without a request nothing changes: a
 * flipped byte in a stored block, or a changed literal that keeps the Huffman stream valid, passes as text.  Plain gzip
 * (one serial stream per file) is out of scope and refused by name.
 *   mm_bgzf_scan_host (no device)  walks the members from data[0]: magic 1f 8b, CM 8, FLG bit 2 (FTEXT may be set, any
 *     other flag is a bad header), the XLEN subfields for BC with SLEN 2 (not necessarily the first), comp_len = BSIZE + 1
 *     - XLEN - 20, ISIZE from the trailer (above 65536: MM_ERR_FORMAT).  It stops at the first incomplete block, when
 *     max_blocks are listed or where *out_bytes would pass max_out_bytes; *consumed = the bytes of the whole blocks taken.
 *     Blocks with ISIZE 0 (the EOF marker, the seams of concatenated files) are consumed and not listed.  comp_off is the
 *     payload's offset in data, out_off the running sum of the listed blocks' isize.  A gzip member without a BC subfield
 *     is MM_ERR_FORMAT with "plain gzip is one serial stream; recompress with bgzip" in mm_last_error(); any other bad
 *     header is MM_ERR_FORMAT.  MM_ERR_NULL: n_blocks, consumed or out_bytes NULL, data NULL with bytes, blocks NULL with
 *     max_blocks != 0.
 *   mm_bgzf_scan_crc_host (no device)  mm_bgzf_scan_host in every respect (one walk serves both), and crcs[i] = the CRC32
 *     of listed block i's trailer (little-endian, the four bytes in front of ISIZE); crcs NULL with max_blocks != 0 is
 *     MM_ERR_NULL.  Blocks with ISIZE 0 are not listed, so THEIR TRAILERS ARE NOT CHECKED by anything that follows.
 *   mm_debug_crc32 (no device)  the gzip CRC32 (zlib's crc32(0, data, n)) of data[0 .. n) by the header's host function;
 *     MM_ERR_NULL for crc NULL, or data NULL with bytes.
 *   mm_bgzf_inflate_device_async  queues ONE launch on the workspace's stream: block b's payload d_comp + comp_off
 *     [comp_len] is inflated to d_out + out_off [isize].  Refused on the host before anything is queued: ws NULL, or with
 *     n_blocks != 0 d_comp, d_blocks or d_out NULL (MM_ERR_NULL); n_blocks >= 2^31 (MM_ERR_LEN_TOO_LARGE).  The table lives
 *     in DEVICE memory, so its entries are checked ON THE DEVICE: an entry beyond comp_bytes or out_capacity (or with isize
 *     above 65536) is not touched, d_status[b] = 100, and mm_workspace_check reports MM_ERR_CAPACITY (kernel error 10).
 *     A block that does not inflate: d_status[b] = its error (csrc/mm_inflate.h, 1..14), mm_workspace_check reports
 *     MM_ERR_FORMAT with "BGZF block" in mm_last_error() (kernel error 9); every other block of the launch is inflated
 *     completely, the failed block's own slot [out_off, out_off + isize) is unspecified and nothing outside it is written.
 *     A launch with both kinds of failure reports the table's: MM_ERR_CAPACITY (the larger kernel error stays).
 *     d_status may be NULL.  No byte outside a block's payload is loaded, none outside its slot stored, whatever the bytes
 *     hold.
 *   mm_bgzf_crc32_device_async  queues ONE launch on the workspace's stream over the same table (only out_off and isize are
 *     read) and the text d_text [text_capacity]: d_crc (may be NULL) receives every block's CRC32; with d_expect (may be
 *     NULL; the trailers' values, from mm_bgzf_scan_crc_host) a block whose CRC32 differs gets d_status[b] = 15, and
 *     mm_workspace_check reports MM_ERR_FORMAT with "CRC32" in mm_last_error() (kernel error 11).  With d_expect, d_status
 *     is also READ: a block whose word is not 0 is skipped - queued behind mm_bgzf_inflate_device_async with the same
 *     array, a block that did not inflate keeps its code and kernel error 9 and is not re-labelled (without an inflate in
 *     front the caller clears the array).  Table entries are checked on the device as above (nothing is read, d_status[b] =
 *     100, d_crc[b] is not written, kernel error 10).  The sticky error word keeps the LARGEST code: a queue with a mismatch
 *     and a bad table entry, or a block that did not inflate, reports the mismatch; d_status tells the blocks apart.
 *     No byte outside [out_off, out_off + isize) is loaded, whatever the alignment.  Refused on the host: ws NULL, d_expect
 *     and d_crc both NULL, or with n_blocks != 0 d_text or d_blocks NULL (MM_ERR_NULL); n_blocks >= 2^31
 *     (MM_ERR_LEN_TOO_LARGE).  d_status may be NULL.
 *   mm_bgzf_inflate_host  scan + upload + kernel + download of a whole BGZF file in host memory: *out_bytes = the text's
 *     size (also with MM_ERR_CAPACITY, when out_capacity is too small: nothing was inflated); a file that ends inside a
 *     block is MM_ERR_FORMAT.
 *   mm_bgzf_inflate_verify_host  the same with every listed block's CRC32 verified: scan with CRCs, upload, inflate with a
 *     status array, the verify launch, download; a mismatch is MM_ERR_FORMAT with "CRC32" in mm_last_error().
 *   mm_debug_bgzf_inflate (no device)  the decoder on the host: one payload into out[0 .. isize); MM_OK or MM_ERR_FORMAT
 *     (mm_last_error() names the decoder's error), MM_ERR_NULL.
 *   mm_fastx_stream_feed_bgzf  serves the unchanged stream handle, DNA and byte text, in place of mm_fastx_stream_feed:
 *     data is a run of BGZF blocks; whole blocks are gathered into a per-slot page-locked compressed staging buffer
 *     (chunk_bytes + 64 KiB, with a device twin; allocated by the first call), and a slot launches when the next block's
 *     ISIZE would pass chunk_bytes, when the staging buffer or the block table (chunk_bytes / 64 + 16 entries, 65536 at
 *     most) is full - so a chunk carries UP TO chunk_bytes new bytes; the table ends a chunk early only where blocks hold
 *     fewer than 64 bytes of text on average (bgzip's hold up to 64 KiB), and such a short chunk may then find no cut for a
 *     record that chunk_bytes would hold: MM_ERR_CAPACITY, "a record longer than chunk_bytes".  The kernel inflates into the slot's text buffer on
 *     the slot's stream in place of the text upload; everything behind it is unchanged, and so is every flag.
 *     *consumed stops behind the last whole block taken - before an incomplete block, or when no slot is free (then call
 *     mm_fastx_stream_next): the caller feeds the rest again, with the bytes that follow it.  mm_fastx_stream_next frees the
 *     slot of the batch it handed out before even when it answers MM_FASTX_NEED_INPUT, so only a second call in a row that
 *     takes nothing, with MM_FASTX_NEED_INPUT in between, says that the rest is the front of an incomplete block (the feed
 *     loops of the Python and C++ mirrors go by this).  mm_fastx_stream_finish after a
 *     call that ended inside a block is MM_ERR_FORMAT (a truncated file): only a later call that takes a whole block
 *     clears that, a call without bytes does not.  A block with ISIZE above chunk_bytes is
 *     MM_ERR_CAPACITY; a bad header or plain gzip MM_ERR_FORMAT as in mm_bgzf_scan_host; a block that does not inflate fails
 *     the stream with MM_ERR_FORMAT; like every stream error these stay.
 *     Format and blank bytes in front: while the format is not known (MM_FASTX_AUTO) and while a FASTQ's first '@' has not
 *     been seen, blocks are inflated on the HOST and their text goes through mm_fastx_stream_feed's own path, so both
 *     behave exactly as for plain text; later blocks go to the device.  mm_fastx_stream_feed may be called BEFORE the
 *     first mm_fastx_stream_feed_bgzf (its bytes stand in front); after it, it is refused with MM_ERR_BAD_MODE.
 *     Offsets (rec_text_pos, text_begin, text_end, first_byte) are offsets in the INFLATED text; BGZF virtual offsets are
 *     out of scope.  A chunk needs a cut like every chunk: keep chunk_bytes well above 64 KiB + the longest record.
 *   MM_FASTX_BGZF_CRC  a flag of mm_fastx_stream_create and mm_fastx_text_stream_create: every block fed through
 *     mm_fastx_stream_feed_bgzf is verified.  A slot keeps the trailers' CRC32s beside its table and uploads them with it,
 *     the inflate gets a status array and the verify launch runs behind it on the slot's stream; a mismatch fails the stream
 *     with MM_ERR_FORMAT, "CRC32" in mm_last_error(), before anything is made of the chunk's text, and like every stream
 *     error it stays.  Blocks inflated on the HOST (above) are checked on the host by the same arithmetic.  Without
 *     mm_fastx_stream_feed_bgzf the flag does nothing.  Which block failed is not reported (the status array stays on the
 *     device).  Per slot: 8 bytes per table entry on the device, 4 page-locked.  The value is 1024: 512 stays an unknown
 *     bit that both creates refuse (MM_ERR_BAD_MODE), as it always was. */
enum { MM_FASTX_BGZF_CRC = 1024 };
typedef struct mm_bgzf_block {
    uint64_t comp_off;   /* offset of the deflate payload in the compressed bytes */
    uint32_t comp_len;   /* its size */
    uint32_t isize;      /* the block's text size, 1 .. 65536 */
    uint64_t out_off;    /* where the text goes in the output */
} mm_bgzf_block_t;
int mm_bgzf_scan_host(const uint8_t *data, uint64_t n_bytes, uint64_t max_blocks, uint64_t max_out_bytes,
                      mm_bgzf_block_t *blocks, uint64_t *n_blocks, uint64_t *consumed, uint64_t *out_bytes);
int mm_bgzf_scan_crc_host(const uint8_t *data, uint64_t n_bytes, uint64_t max_blocks, uint64_t max_out_bytes,
                          mm_bgzf_block_t *blocks, uint64_t *n_blocks, uint64_t *consumed, uint64_t *out_bytes,
                          uint32_t *crcs /* [max_blocks] */);
int mm_debug_crc32(const uint8_t *data, uint64_t n, uint32_t *crc);
int mm_bgzf_inflate_device_async(mm_workspace_t *ws, const void *d_comp, uint64_t comp_bytes,
                                 const mm_bgzf_block_t *d_blocks, uint64_t n_blocks, void *d_out, uint64_t out_capacity,
                                 uint32_t *d_status /* [n_blocks] or NULL */);
int mm_bgzf_inflate_host(mm_workspace_t *ws, const uint8_t *data, uint64_t n_bytes, uint8_t *out, uint64_t out_capacity,
                         uint64_t *out_bytes);
int mm_bgzf_crc32_device_async(mm_workspace_t *ws, const void *d_text, uint64_t text_capacity,
                               const mm_bgzf_block_t *d_blocks, uint64_t n_blocks, const uint32_t *d_expect /* or NULL */,
                               uint32_t *d_crc /* [n_blocks] or NULL */, uint32_t *d_status /* [n_blocks] or NULL */);
int mm_bgzf_inflate_verify_host(mm_workspace_t *ws, const uint8_t *data, uint64_t n_bytes, uint8_t *out,
                                uint64_t out_capacity, uint64_t *out_bytes);
int mm_debug_bgzf_inflate(const uint8_t *payload, uint32_t comp_len, uint8_t *out, uint32_t isize);
int mm_fastx_stream_feed_bgzf(mm_fastx_stream_t *s, const uint8_t *data, uint64_t n_bytes, uint64_t *consumed);
/* ------------------------------------------------------------------ several devices from one call
 * The reference's parallel driver is host code: rayon over the contigs, one Builder::run each
 * (bench/src/bin/paper.rs:442-459).  A device group holds one workspace (stream, scratch) per listed device; a
 * device may be listed more than once.  Both calls run one host thread per entry, keep the count exchange on
 * the host (nothing crosses between the devices) and deliver ONE dense result in the caller's host buffers. */
int mm_device_group_create(mm_device_group_t **out, const int *devices, int n_devices);
void mm_device_group_destroy(mm_device_group_t *group);
int mm_device_group_size(const mm_device_group_t *group);
/* One sequence cut into n equal window ranges, one per entry of the group: absolute positions, exact seam (a
 * range starts by comparing with the window before it, which is the reference's rule for joining lanes,
 * src/collect.rs:265-271; syncmers have no such rule).  Same result as mm_run_host.  MM_ERR_CAPACITY: *out_count
 * holds the need. */
int mm_run_sharded_host(const mm_plan_t *plan, mm_device_group_t *group, const uint8_t *packed,
                        uint64_t base_offset, uint64_t n_bases, uint32_t *out_pos, uint32_t *out_sk /* or NULL */,
                        uint64_t capacity, uint64_t *out_count);
/* n_seqs independent sequences (contigs) placed greedily, longest first, on the entries of the group; every
 * entry runs its sequences in one batch launch.  Positions are sequence-local and lie in input order:
 * sequence s = out_pos[out_offsets[s] .. out_offsets[s + 1]).  Same result as mm_run_batch_device. */
int mm_run_batch_sharded_host(const mm_plan_t *plan, mm_device_group_t *group, uint64_t n_seqs,
                              const uint8_t *const *packed, const uint64_t *base_offsets /* or NULL */,
                              const uint64_t *n_bases, uint32_t *out_pos, uint32_t *out_sk /* or NULL */,
                              uint64_t capacity, uint64_t *out_offsets /* [n_seqs + 1] */);

/* ---- device-resident shards (round 4).  north_star's multi-GPU shape: the sequence already lives in HBM, every
 * device walks its window range with one asynchronous launch, the positions STAY on their devices, and "at most" a
 * gather moves them to one device over xGMI.  No host buffers, no PCIe transfer, no host thread per device.
 *
 * The sequence: mm_device_group_upload copies the caller's packed bytes to every device of the group ONCE (kept
 * until the next upload or the group's end); mm_device_group_adopt takes device pointers the caller already
 * holds instead - d_packed[i] on the device of entry i, each addressing the same packed_bytes of the same
 * sequence, not owned by the group.  (Every entry addresses the whole sequence so that positions are absolute;
 * an entry only READS the bytes of its own window range and a halo of k + w - 1 bases.) */
int mm_device_group_upload(mm_device_group_t *group, const uint8_t *packed, uint64_t packed_bytes);
/* The same for ONE run shape: every entry receives only the bytes its window range of an N-way split of
 * (base_offset, n_bases) can read - its share plus a halo that covers any k + w - 1 below 2^17 - so the sequence crosses
 * the host link once in total, not once per device (the whole extent is still allocated on every device: offsets stay
 * absolute).  mm_run_sharded_device refuses (MM_ERR_NULL, mm_last_error() names the ranges) a run whose shape needs bytes
 * an entry does not hold.  MM_ERR_CAPACITY: the bases do not fit packed_bytes. */
int mm_device_group_upload_range(mm_device_group_t *group, const uint8_t *packed, uint64_t packed_bytes,
                                 uint64_t base_offset, uint64_t n_bases);
int mm_device_group_adopt(mm_device_group_t *group, const void *const *d_packed /* [size] */, uint64_t packed_bytes);
/* Builder::run over the resident sequence, cut into mm_device_group_size(group) equal window ranges (absolute
 * positions, exact seam: range i starts by comparing with the window before it, src/collect.rs:265-271, so the
 * shards laid end to end ARE the single-device result).  One asynchronous launch per entry, issued from the
 * calling thread; the call returns when all have finished.  The positions (and super-k-mer indices when
 * want_superkmers != 0) are left in result buffers the group owns and grows, one per entry: see
 * mm_device_group_result.  counts[i] (may be NULL) receives entry i's count, *total (may be NULL) their sum. */
int mm_run_sharded_device(const mm_plan_t *plan, mm_device_group_t *group, uint64_t base_offset, uint64_t n_bases,
                          int want_superkmers, uint64_t *counts /* [size] or NULL */, uint64_t *total);
/* Entry i's shard of the last mm_run_sharded_device: device pointers on that entry's device (valid until the next
 * run on the group), its count and its window range.  Any out pointer may be NULL. */
int mm_device_group_result(const mm_device_group_t *group, int entry, uint32_t **d_pos, uint32_t **d_sk,
                           uint64_t *count, uint64_t *win_begin, uint64_t *win_end);
/* The optional exchange: the shards of the last run, dense and in window order, into d_dst_pos (and d_dst_sk) on
 * the device of entry `root` - device-to-device copies (hipMemcpyPeerAsync: over xGMI between the GPUs of a node),
 * all in flight together; no RCCL dependency.  *total receives the number of positions; MM_ERR_CAPACITY when they
 * do not fit `capacity` (nothing is copied then).  The copies run on the SOURCE entries' streams and the call waits for
 * them; they are not ordered against work the caller has queued on the destination: d_dst_pos / d_dst_sk must be idle
 * (no kernel or copy of the caller's still reading or writing them) when this is called.  MM_ERR_NULL when the group's
 * last run was a batch run (mm_run_batch_sharded_device: see mm_device_group_gather_batch) - the two resident modes
 * share the result buffers, each call invalidates the other mode's results. */
int mm_device_group_gather(mm_device_group_t *group, int root, uint32_t *d_dst_pos, uint32_t *d_dst_sk /* or NULL */,
                           uint64_t capacity, uint64_t *total);

/* ---- device-resident BATCHES (round 4): north_star's "sharded by contig across the GPUs of a node, gather of the
 * positions".  mm_device_group_upload_batch places n_seqs independent sequences greedily, longest first, on the
 * entries of the group and copies each to ITS entry's device only (kept until the next batch upload / the group's
 * end).  mm_run_batch_sharded_device runs every entry's sequences in ONE batch launch on its device (Builder::run per
 * sequence, sequence-local positions, bench/src/bin/paper.rs:425-431,442-459); the positions stay on the devices.
 * n_bases[s] (and base_offsets[s], or NULL) describe sequence s of the upload; out_counts[s] (may be NULL) receives
 * its count, *total their sum.  mm_device_group_batch_result hands out where a sequence's positions lie;
 * mm_device_group_gather_batch copies all sequences, in input order, into device memory of entry `root`
 * (device-to-device) and fills the n_seqs + 1 offsets.  Like mm_run_sharded_device the run issues one asynchronous
 * launch per entry from the calling thread and then waits for them in turn (round 5; round 4 ran a host thread per
 * entry); its destination rule for the gather is mm_device_group_gather's. */
int mm_device_group_upload_batch(mm_device_group_t *group, uint64_t n_seqs, const uint8_t *const *packed,
                                 const uint64_t *packed_bytes);
int mm_run_batch_sharded_device(const mm_plan_t *plan, mm_device_group_t *group, const uint64_t *base_offsets /* or NULL */,
                                const uint64_t *n_bases, int want_superkmers, uint64_t *out_counts /* [n_seqs] or NULL */,
                                uint64_t *total);
int mm_device_group_batch_result(const mm_device_group_t *group, uint64_t seq, int *entry, uint32_t **d_pos,
                                 uint32_t **d_sk, uint64_t *count);
int mm_device_group_gather_batch(mm_device_group_t *group, int root, uint32_t *d_dst_pos, uint32_t *d_dst_sk /* or NULL */,
                                 uint64_t capacity, uint64_t *out_offsets /* [n_seqs + 1] */);
/* Output::values_u64 / values_u128 (src/lib.rs:584-629) of the positions of the last mm_run_batch_sharded_device, in place
 * of Output::values_* per contig of the loop bench/src/bin/paper.rs:410-431: ONE launch of the batch values kernel per
 * entry over its resident sequences and result positions (the group owns the uploaded copies, so no per-sequence call could
 * reach them).  The launches are issued from the calling thread one after the other and then waited for; the values land in
 * a buffer the group owns on the entry's device.  len / canonical as for mm_values_u64_device_async; want_u128: {lo, hi}
 * per value.  *total (may be NULL) receives the number of values.  MM_ERR_NULL without a finished batch run.
 * mm_device_group_batch_values hands out where sequence seq's values lie: *d_values on the device of *entry, *count values
 * (2 * *count words after want_u128).  The next upload or run on the group invalidates them (MM_ERR_NULL until the next
 * mm_device_group_values_batch).  Out of scope: a gather of the values across devices. */
int mm_device_group_values_batch(mm_device_group_t *group, uint32_t len, int canonical, int want_u128, uint64_t *total);
int mm_device_group_batch_values(const mm_device_group_t *group, uint64_t seq, int *entry, uint64_t **d_values,
                                 uint64_t *count);

/* Diagnostics: the launch plan of the fused kernel as the host lays it out - lane length, tiles, the tapered tail
 * (DESIGN.md 4.1 "Launch geometry").  With MM_TAPER_SLOTS=<workgroup slots> in the environment no device is needed:
 * the CPU test-suite checks with it that the tiles tile every window range exactly.  n_seqs == 0: ONE sequence of
 * n_windows[0] windows, out7 = {blocks per lane, tiles, first tapered tile, tiles per taper level, last level's blocks
 * per lane, first tapered window, windows per block of a tile}.  n_seqs > 0: a batch, the tile table itself (tile t =
 * sequence, first window, blocks per lane; out7[0] = the longest lane); MM_ERR_CAPACITY when it holds more than
 * tile_capacity tiles (*n_tiles says how many).  mode: 0 minimizers, 1 / 2 closed / open syncmers, 3 minimizers with
 * super-k-mer indices (whose 16-bit list entries bound the lanes), 4 minimizers over a PackedNSeq (the skip-ambiguous walk's
 * lane rules).  With MM_TAPER_SLOTS set the single-sequence plan also applies the one-round rule (a run of 0.6 .. 1 round of
 * that many slots gets one tile per slot).
 * mm_debug_launch_lds: the dynamic LDS of the same single-sequence launch, out2 = {bytes of the lane lists, bytes of the
 * skip-ambiguous walk's landing area in front of them (0 without ambiguity bits)} - the CPU suite checks that the two fit
 * the CU as often as the kernel's register bound lets workgroups share it. */
int mm_debug_launch_plan(uint32_t w, int canonical_windows, int mode, uint64_t n_seqs, const uint64_t *n_windows,
                         uint64_t *out7, uint32_t *tile_seq, uint32_t *tile_win0, uint32_t *tile_nblk,
                         uint64_t tile_capacity, uint64_t *n_tiles);
int mm_debug_launch_lds(uint32_t w, int canonical_windows, int mode, uint64_t n_windows, uint64_t *out2);
/* Diagnostics: 1 when a minimizer run (positions only) of one sequence or a batch of sequences with this (k, w) and window
 * flavour is launched with a kernel compiled for that k (one sequence load stream), 0 when it takes the
 * kernel that reads k at run time.  Both compute the same; the GPU test-suite checks that.  No device needed.  One of the
 * mm_debug_* family: for tests and tools, no part of the drop-in interface.  In the EXPERIMENTS build of the library the
 * answer follows its switches - MM_NO_KC, MM_JIT_FORCE and a non-zero MM_DEBUG all make it 0. */
int mm_debug_fixed_k_kernel(uint32_t k, uint32_t w, int canonical_windows);
/* Diagnostics: the strand count of a tied window as the fixed-k canonical walk makes it.  That walk keeps no
 * running count: where a window's leftmost and rightmost minimum differ it counts the window's T|G bases from the two
 * byte-aligned sequence buffers it holds in registers, through a compile-time plan of at most three pieces per (kn, jj) - kn the
 * index of the NEXT block within its load group, jj the step within the block.  This call runs the same plan on the host: it
 * builds the two buffers as a lane does whose first k-mer begins at base lane_base (-1: the base before the buffer) of the
 * packed bytes (4 bases per byte, low bits first; bytes past n_bytes read as 0) and counts the window decided at step jj of
 * block 1 + kn + group * (blocks per load group), i.e. the k + w - 1 bases from lane_base + (kn + group * blocks) * w + jj + 1
 * on.  Returns a bit mask: 1 - (w, k) walks with one load stream; 2 - ... and counts tied windows by such a plan; 4 - *count
 * was written (needs bit 2, bytes, count, kn below the blocks per group, jj < w, lane_base >= -1).  No device needed. */
int mm_debug_kc_count(uint32_t w, uint32_t k, uint32_t kn, uint32_t jj, uint32_t group, const uint8_t *bytes,
                      uint64_t n_bytes, int64_t lane_base, uint32_t *count);
/* Diagnostics: the pair table of the fixed-k canonical walk (k=21 w=11), made on the host by the function the
 * kernel's threads run.  That walk looks its rolling-hash contributions up two bases at a time: entry i = in4 | out4 << 4 -
 * in4 / out4 the 2-bit codes of two consecutive bases entering / leaving the hash, first base in the low bits - is
 * out[4 i .. 4 i + 3] = {t1.fw, t1.rc, rotl(t1.fw, rot) ^ t2.fw, rotr(t1.rc, rot) ^ t2.rc} with t1 / t2 the one-base
 * contributions (in ^ out terms) of the first / second base pair, for the hasher's tables at k = 21.  Two one-base steps
 * from any state equal the pair step; the CPU test-suite checks that.  MM_ERR_NULL for a null argument.  No device needed. */
int mm_debug_pair_table(const mm_hasher_t *h, uint32_t out[1024]);
/* Diagnostics: what the fused kernel's walk decides at COMPILE time from its window size, for one flavour - window strand,
 * mode (0 minimizers, 1 / 2 closed / open syncmers), super-k-mer indices, reads mode, the skip-ambiguous walk.  Every window
 * size up to 128 is a kernel of its own (prebuilt, or compiled at first use), and the kernel source branches on the window size in
 * these places; the values come from the constexpr functions the kernel itself calls, so the test-suite
 * can tell which window sizes are the same combination of branches and check that it runs each combination.  Writes
 * min(capacity, MM_WALK_TRAITS) values to out (may be null with capacity 0) in the order below and returns MM_WALK_TRAITS;
 * 0 for w == 0 or a mode out of range.  No device needed.  MM_TRAIT_LAST_VIEW_BASES - the bases in the last 16-base view of a
 * block, plus the strand window's extra base for canonical windows - takes every value from 1 to 17 within one
 * combination of the others: it names the edge a window size sits at, not a branch. */
#define MM_TRAIT_WIDE_GROUP_BLOCKS 0 /* blocks that share one wide sequence load (0: 8-byte loads per block) */
#define MM_TRAIT_WIDE_DWORDS 1       /* dwords of a wide load, 4 or 5 */
#define MM_TRAIT_V2_LOAD 2           /* the strand window's leaving base has a load stream of its own */
#define MM_TRAIT_VIEW_WORDS 3        /* 16-base view words per block, ceil(w / 16) */
#define MM_TRAIT_AMB_VIEW_WORDS 4    /* 32-window words of ambiguity bits per block (1 without them) */
#define MM_TRAIT_SK_SHIFT 5          /* shift of the packed super-k-mer list entries (0 without indices) */
#define MM_TRAIT_AMBI_LAND 6         /* the skip-ambiguous look-ahead lands in LDS */
#define MM_TRAIT_AMBI_ROWS 7         /* ... and the window bits arrive in chunks of rows */
#define MM_TRAIT_AMB_ROW_DWORDS 8    /* rows of such a chunk (0 without chunks) */
#define MM_TRAIT_LAZY_VOTE 9         /* the strand vote is resolved only where a window ties */
#define MM_TRAIT_TABLE_PREFETCH 10   /* steps the hash-table look-ups run ahead */
#define MM_TRAIT_TWO_BODIES 11       /* partial walks carry a fast and a flag body per block */
#define MM_TRAIT_ENTRY8 12           /* 8-bit list entries */
#define MM_TRAIT_ONE_STREAM 13       /* one sequence load stream (always 0 here: k is read at run time) */
#define MM_TRAIT_LAST_VIEW_BASES 14
#define MM_WALK_TRAITS 15
int mm_debug_walk_traits(uint32_t w, int canonical_windows, int mode, int super_kmers, int reads, int ambiguous,
                         uint32_t *out, int capacity);
/* Diagnostics of the lane-table launches (round 6).  mm_debug_lane_plan: the lane length and grid the host
 * chooses for n_reads reads of total_bases bases - out6 = {blocks per lane, windows per lane S, entries per lane list, bytes of
 * the lane lists, upper bound of the lanes (a multiple of 256), tiles}; mode as in mm_debug_launch_plan (3: with super-k-mer
 * indices, whose packed 16-bit entries bound S; 4: over a PackedNSeq); blocks_per_lane 0 = the default.  No device needed.
 * mm_debug_last_lane_table: copies the table the workspace's LAST lane-table run built to the host - lane i =
 * {start, win0, count, read} in out4[4 i .. 4 i + 3] - up to `capacity` lanes; *n_lanes = lanes of the (padded) table.  The
 * GPU test-suite checks with it that the lanes tile every read's windows exactly. */
int mm_debug_lane_plan(uint32_t k, uint32_t w, int canonical_windows, int mode, uint64_t n_reads, uint64_t total_bases,
                       uint32_t blocks_per_lane, uint64_t *out6);
int mm_debug_last_lane_table(mm_workspace_t *ws, uint32_t *out4, uint64_t capacity, uint64_t *n_lanes);
/* Diagnostics: the shader clock while other work runs on the device.  _begin starts a handful of sleeping
 * single-wave workgroups on a stream of the workspace's own that sample the shader cycle counter against the
 * 100 MHz real-time counter for duration_us; _end waits for them and returns the mean clock in GHz (bench.py
 * brackets its timed loop with the pair: the VALU bound of roofline.valu is priced at THIS clock). */
/* Diagnostics: the host link of this box - host -> device alone, device -> host alone and BOTH AT ONCE (copy engines, two
 * streams), `bytes` each way between the caller's (page-locked) buffers and device memory the call allocates.
 * out_GBps[0..2] = the two one-way rates and the SUM of both directions while they run together; the floor of
 * mm_run_host follows from the third, which is less than the sum of the first two (bench.py: end_to_end.link). */
int mm_link_probe(mm_workspace_t *ws, const void *host_in, void *host_out, uint64_t bytes, double *out_GBps /* [3] */);
int mm_clock_probe_begin(mm_workspace_t *ws, uint64_t duration_us);
int mm_clock_probe_end(mm_workspace_t *ws, double *ghz);
/* Deterministic synthetic PackedSeq generator G of BASELINE.md §4, written on the device. */
int mm_generate_device_async(mm_workspace_t *ws, uint64_t seed, uint64_t first_base,
                             uint64_t n_bases, uint8_t *d_packed /* ceil(n/4) bytes */);

#ifdef __cplusplus
}
#endif
#endif
