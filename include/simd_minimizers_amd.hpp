// simd_minimizers_amd.hpp — header-only C++ mirror of the reference's builder API
// (rust-seq/simd-minimizers src/lib.rs:225-654) over the C ABI of simd_minimizers_amd.h.
//
//   using namespace simd_minimizers;
//   std::vector<uint32_t> pos, sk;
//   auto out = canonical_minimizers(21, 11).super_kmers(&sk).run(PackedSeq{bytes, 0, n}, pos);
//   std::vector<uint64_t> vals = out.values_u64();
//
// Names, argument meaning and error behaviour follow the reference: `run` APPENDS to the
// output vector (src/lib.rs:80-81) and drops a leading result equal to its previous last
// element (src/collect.rs:265-271); the reference's assert!/panic! conditions surface as
// simd_minimizers::Error carrying the MM_ERR_* code.  All compute happens in the HIP library.
#pragma once
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "simd_minimizers_amd.h"

namespace simd_minimizers {

struct Error : std::runtime_error {
    int code;
    Error(int c) : std::runtime_error(std::string(mm_strerror(c)) + " " + mm_last_error()), code(c) {}
};
inline void check(int c) {
    if (c != MM_OK) throw Error(c);
}

// packed-seq PackedSeq: borrowed view of 2-bit bases (A0 C1 T2 G3, 4 per byte)
struct PackedSeq {
    const uint8_t *data;
    uint64_t offset;  // first base inside `data`
    uint64_t len;
    PackedSeq slice(uint64_t b, uint64_t e) const { return PackedSeq{data, offset + b, e - b}; }
};
// packed-seq PackedNSeq: a PackedSeq plus one ambiguity bit per base (bit (amb_offset+i)%8 of byte
// (amb_offset+i)/8 of `amb`)
struct PackedNSeq {
    PackedSeq seq;
    const uint8_t *amb;
    uint64_t amb_offset;
    PackedNSeq slice(uint64_t b, uint64_t e) const { return PackedNSeq{seq.slice(b, e), amb, amb_offset + b}; }
};
// packed-seq AsciiSeq: ACTG / actg characters
struct AsciiSeq {
    const uint8_t *data;
    uint64_t len;
};

// general byte text, the reference's &[u8] (src/lib.rs:59): one character per byte, all 256 values legal
struct TextSeq {
    const uint8_t *data;
    uint64_t len;
};

// seq-hash NtHasher<CANONICAL>::new(k)
template <bool CANONICAL = true>
struct NtHasher {
    mm_hasher_t tables;
    uint32_t k;
    explicit NtHasher(uint32_t k_) : k(k_) { check(mm_default_hasher(&tables, CANONICAL)); }
    bool is_canonical() const { return CANONICAL; }
};
// seq-hash MulHasher<CANONICAL>::new(k) / AntiLexHasher<CANONICAL>::new(k) (src/lib.rs:71-72; src/test.rs:81-83,
// 107-109).  PARITY UNPINNED: their arithmetic is not in the reference tree (see mm_mul_hasher /
// mm_antilex_hasher in the C header); a caller who knows the real per-base values fills `tables` itself.
template <bool CANONICAL = true>
struct MulHasher {
    mm_hasher_t tables;
    uint32_t k;
    explicit MulHasher(uint32_t k_) : k(k_) { check(mm_mul_hasher(&tables, CANONICAL)); }
    bool is_canonical() const { return CANONICAL; }
};
template <bool CANONICAL = true>
struct AntiLexHasher {
    mm_hasher_t tables;
    uint32_t k;
    explicit AntiLexHasher(uint32_t k_) : k(k_) { check(mm_antilex_hasher(&tables, k_, CANONICAL)); }
    bool is_canonical() const { return CANONICAL; }
};

// MulHasher<CANONICAL>::new(k) over bytes, the default of &[u8] text (src/lib.rs:71-72; PARITY UNPINNED, see
// mm_text_mul_hasher).  Any mm_text_hasher_t - mm_text_hasher_from_dna of an NtHasher, tables of the caller's own -
// goes to Builder::hasher as well.
template <bool CANONICAL = true>
struct TextMulHasher {
    mm_text_hasher_t tables;
    uint32_t k;
    explicit TextMulHasher(uint32_t k_) : k(k_) { check(mm_text_mul_hasher(&tables, CANONICAL)); }
    bool is_canonical() const { return CANONICAL; }
};

class Workspace {
  public:
    explicit Workspace(int device = 0, void *stream = nullptr) { check(mm_workspace_create(&ws_, device, stream)); }
    ~Workspace() { mm_workspace_destroy(ws_); }
    Workspace(const Workspace &) = delete;
    Workspace &operator=(const Workspace &) = delete;
    mm_workspace_t *get() const { return ws_; }
    // the completion half of the asynchronous calls (mm_workspace_check): waits for the stream, throws what they raised
    void check_async() { check(mm_workspace_check(ws_)); }
    static Workspace &thread_default() {  // the reference's thread_local CACHE (src/lib.rs:217-219)
        thread_local Workspace w;
        return w;
    }

  private:
    mm_workspace_t *ws_ = nullptr;
};

using u128 = unsigned __int128;

template <bool CANONICAL>
class Output {  // src/lib.rs:232-237
  public:
    Output(uint32_t len, PackedSeq seq, const std::vector<uint32_t> *pos, Workspace *ws)
        : len_(len), seq_(seq), pos_(pos), ws_(ws) {}
    std::vector<uint64_t> values_u64() const {  // src/lib.rs:584-612
        std::vector<uint64_t> v(pos_->size());
        check(mm_values_u64_host(ws_->get(), seq_.data, seq_.offset, seq_.len, len_, CANONICAL, pos_->data(),
                                 pos_->size(), v.data()));
        return v;
    }
    std::vector<u128> values_u128() const {  // src/lib.rs:587-593 (len <= 64)
        std::vector<uint64_t> raw(2 * pos_->size());
        check(mm_values_u128_host(ws_->get(), seq_.data, seq_.offset, seq_.len, len_, CANONICAL, pos_->data(),
                                  pos_->size(), raw.data()));
        std::vector<u128> v(pos_->size());
        for (size_t i = 0; i < v.size(); ++i) v[i] = ((u128)raw[2 * i + 1] << 64) | raw[2 * i];
        return v;
    }
    std::vector<std::pair<uint32_t, uint64_t>> pos_and_values_u64() const {  // src/lib.rs:598-612
        const std::vector<uint64_t> v = values_u64();
        std::vector<std::pair<uint32_t, uint64_t>> r(v.size());
        for (size_t i = 0; i < v.size(); ++i) r[i] = {(*pos_)[i], v[i]};
        return r;
    }
    std::vector<std::pair<uint32_t, u128>> pos_and_values_u128() const {  // src/lib.rs:615-630
        const std::vector<u128> v = values_u128();
        std::vector<std::pair<uint32_t, u128>> r(v.size());
        for (size_t i = 0; i < v.size(); ++i) r[i] = {(*pos_)[i], v[i]};
        return r;
    }
    const std::vector<uint32_t> &positions() const { return *pos_; }

  private:
    uint32_t len_;
    PackedSeq seq_;
    const std::vector<uint32_t> *pos_;
    Workspace *ws_;
};

template <bool CANONICAL, int SYNCMER>
class Builder {  // src/lib.rs:225-230
  public:
    Builder(uint32_t k, uint32_t w) : k_(k), w_(w) {}
    template <class H>
    Builder hasher(const H &h) const {  // src/lib.rs:327 (any KmerHasher: NtHasher, MulHasher, AntiLexHasher)
        Builder b = *this;
        b.hasher_ = h.tables;
        b.has_hasher_ = true;
        return b;
    }
    // the hasher of byte text (TextSeq runs); the hasher of 2-bit sequences is kept
    Builder hasher(const mm_text_hasher_t &h) const {
        Builder b = *this;
        b.text_hasher_ = h;
        b.has_text_hasher_ = true;
        return b;
    }
    template <bool C>
    Builder hasher(const TextMulHasher<C> &h) const {
        return hasher(h.tables);
    }
    Builder super_kmers(std::vector<uint32_t> *sk) const {  // src/lib.rs:341 (minimizers only)
        static_assert(SYNCMER == 0, "super_kmers() is only defined for minimizers");
        Builder b = *this;
        b.sk_ = sk;
        return b;
    }
    Builder workspace(Workspace *ws) const {
        Builder b = *this;
        b.ws_ = ws;
        return b;
    }
    // The reference's `run` (src/lib.rs:378) is compiled code: its first call costs what every call costs.  Here a
    // builder's first run loads - and for some (flavour, w) compiles - its kernels; prepare() does that part ahead of
    // the first run, on this builder's workspace, and launches nothing (mm_plan_prepare).  `what`: MM_PREPARE_SEQUENCE
    // for run / run_scalar / run_once, MM_PREPARE_READS for run_many; a builder with .super_kmers() prepares those
    // kernels as well.  Returns the report: kernels looked at, compiled, loaded from the disk cache, unavailable.
    mm_prepare_report_t prepare(unsigned what = MM_PREPARE_SEQUENCE) const {
        Workspace &ws = ws_ ? *ws_ : Workspace::thread_default();
        mm_plan_t *plan = make_plan();
        mm_prepare_report_t rep{0, 0, 0, 0};
        const int r = mm_plan_prepare(plan, ws.get(), what | (sk_ && what ? (unsigned)MM_PREPARE_SUPERKMERS : 0u), &rep);
        mm_plan_destroy(plan);
        check(r);
        return rep;
    }
    Output<CANONICAL> run(PackedSeq seq, std::vector<uint32_t> &min_pos) const {  // src/lib.rs:378
        Workspace &ws = ws_ ? *ws_ : Workspace::thread_default();
        std::vector<uint32_t> pos, sk;
        const uint64_t n = compute(seq, ws, pos, sk);
        size_t first = 0;
        if (SYNCMER == 0)
            while (first < n && !min_pos.empty() && pos[first] == min_pos.back()) ++first;
        min_pos.insert(min_pos.end(), pos.begin() + first, pos.begin() + n);
        if (sk_) sk_->insert(sk_->end(), sk.begin() + first, sk.begin() + n);
        return Output<CANONICAL>(SYNCMER ? k_ + w_ - 1 : k_, seq, &min_pos, &ws);
    }
    // src/lib.rs:553-576: `run` with the scratch passed explicitly; the reference's Cache is this
    // engine's Workspace (device buffers + stream)
    Output<CANONICAL> run_with_buf(PackedSeq seq, std::vector<uint32_t> &min_pos, Workspace &cache) const {
        return workspace(&cache).run(seq, min_pos);
    }
    // src/lib.rs:370-376, :517-543.  The reference's scalar collectors OVERWRITE min_pos from index 0
    // and truncate it to the result (src/collect.rs:15-37,39-76, src/syncmers.rs:19-48): no append, no
    // last() rule; a sequence without a window clears min_pos and leaves the super-k-mer vector
    // untouched (src/collect.rs:45-48).  Served by the same HIP kernel as `run`.
    Output<CANONICAL> run_scalar(PackedSeq seq, std::vector<uint32_t> &min_pos) const {
        Workspace &ws = ws_ ? *ws_ : Workspace::thread_default();
        std::vector<uint32_t> pos, sk;
        const uint64_t n = compute(seq, ws, pos, sk);
        min_pos.assign(pos.begin(), pos.begin() + n);
        if (sk_ && seq.len >= (uint64_t)k_ + w_ - 1) sk_->assign(sk.begin(), sk.begin() + n);
        return Output<CANONICAL>(SYNCMER ? k_ + w_ - 1 : k_, seq, &min_pos, &ws);
    }
    std::vector<uint32_t> run_scalar_once(PackedSeq seq) const {  // src/lib.rs:358-362, :511-515
        std::vector<uint32_t> v;
        run_scalar(seq, v);
        return v;
    }
    // src/lib.rs:451-496: canonical builders only; windows with an ambiguous base are skipped
    Output<CANONICAL> run_skip_ambiguous_windows(PackedNSeq nseq, std::vector<uint32_t> &min_pos) const {
        static_assert(CANONICAL, "run_skip_ambiguous_windows() is only defined for canonical builders");
        Workspace &ws = ws_ ? *ws_ : Workspace::thread_default();
        mm_plan_t *plan = nullptr;
        check(mm_plan_create(&plan, k_, w_, CANONICAL, (mm_mode_t)SYNCMER, has_hasher_ ? &hasher_ : nullptr));
        const uint64_t l = (uint64_t)k_ + w_ - 1;
        const uint64_t cap = nseq.seq.len >= l ? nseq.seq.len - l + 1 : 0;
        std::vector<uint32_t> pos(cap ? cap : 1);
        uint64_t n = 0;
        int r = mm_run_skip_ambiguous_host(plan, ws.get(), nseq.seq.data, nseq.seq.offset, nseq.amb,
                                           nseq.amb_offset, nseq.seq.len, pos.data(), cap, &n);
        mm_plan_destroy(plan);
        check(r);
        size_t first = 0;
        if (SYNCMER == 0)
            while (first < n && !min_pos.empty() && pos[first] == min_pos.back()) ++first;
        min_pos.insert(min_pos.end(), pos.begin() + first, pos.begin() + n);
        return Output<CANONICAL>(SYNCMER ? k_ + w_ - 1 : k_, nseq.seq, &min_pos, &ws);
    }
    Output<CANONICAL> run_skip_ambiguous_windows_with_buf(PackedNSeq nseq, std::vector<uint32_t> &min_pos,
                                                          Workspace &cache) const {  // src/lib.rs:465-496
        return workspace(&cache).run_skip_ambiguous_windows(nseq, min_pos);
    }
    std::vector<uint32_t> run_skip_ambiguous_windows_once(PackedNSeq nseq) const {
        std::vector<uint32_t> v;
        run_skip_ambiguous_windows(nseq, v);
        return v;
    }
    std::vector<uint32_t> run_once(PackedSeq seq) const {  // src/lib.rs:364
        std::vector<uint32_t> v;
        run(seq, v);
        return v;
    }
    // src/lib.rs:378 on &[u8] text (mm_run_text_host): positions are APPENDED to min_pos with the last() rule.
    // (No Output: the k-mer values of the positions come from values_u64 / values_u128 (TextSeq, pos, encoding) below.)
    std::vector<uint32_t> &run(TextSeq seq, std::vector<uint32_t> &min_pos) const {
        Workspace &ws = ws_ ? *ws_ : Workspace::thread_default();
        mm_plan_t *plan = nullptr;
        check(mm_plan_create_text(&plan, k_, w_, CANONICAL, (mm_mode_t)SYNCMER,
                                  has_text_hasher_ ? &text_hasher_ : nullptr));
        const uint64_t l = (uint64_t)k_ + w_ - 1;
        const uint64_t cap = seq.len >= l ? seq.len - l + 1 : 0;
        std::vector<uint32_t> pos(cap ? cap : 1), sk(sk_ && cap ? cap : 1);
        uint64_t n = 0;
        int r = mm_run_text_host(plan, ws.get(), seq.data, seq.len, pos.data(), sk_ ? sk.data() : nullptr, cap, &n);
        mm_plan_destroy(plan);
        check(r);
        size_t first = 0;
        if (SYNCMER == 0)
            while (first < n && !min_pos.empty() && pos[first] == min_pos.back()) ++first;
        min_pos.insert(min_pos.end(), pos.begin() + first, pos.begin() + n);
        if (sk_) sk_->insert(sk_->end(), sk.begin() + first, sk.begin() + n);
        return min_pos;
    }
    std::vector<uint32_t> run_once(TextSeq seq) const {
        std::vector<uint32_t> v;
        run(seq, v);
        return v;
    }
    std::vector<uint32_t> run_once(AsciiSeq seq) const {
        Workspace &ws = ws_ ? *ws_ : Workspace::thread_default();
        mm_plan_t *plan = nullptr;
        check(mm_plan_create(&plan, k_, w_, CANONICAL, (mm_mode_t)SYNCMER, has_hasher_ ? &hasher_ : nullptr));
        const uint64_t l = (uint64_t)k_ + w_ - 1;
        const uint64_t cap = seq.len >= l ? seq.len - l + 1 : 0;
        std::vector<uint32_t> pos(cap ? cap : 1);
        uint64_t n = 0;
        int r = mm_run_host_ascii(plan, ws.get(), seq.data, seq.len, pos.data(), nullptr, cap, &n);
        mm_plan_destroy(plan);
        check(r);
        pos.resize(n);
        return pos;
    }

    // MANY sequences in ONE call (round 6) - what a caller that loops `run` over its reads does instead (src/lib.rs:378
    // per read; the reference's `short` experiment, bench/src/bin/paper.rs:62-115): the reads are packed back to back on
    // the host, one upload, ONE launch whatever their lengths (a read longer than a lane takes consecutive lanes of the
    // device-built lane table), one download.  Positions are read-local; read r's are pos[offsets[r] .. offsets[r + 1]).
    // With .super_kmers(&sk) the indices come back the same way.  pos / offsets / sk are OVERWRITTEN.
    void run_many(const std::vector<PackedSeq> &reads, std::vector<uint32_t> &pos, std::vector<uint64_t> &offsets) const {
        Workspace &ws = ws_ ? *ws_ : Workspace::thread_default();
        std::vector<uint64_t> starts(reads.size() + 1, 0);
        uint32_t longest = 0;
        for (size_t r = 0; r < reads.size(); ++r) {
            starts[r + 1] = starts[r] + reads[r].len;
            if (reads[r].len > longest) longest = (uint32_t)reads[r].len;
        }
        const uint64_t total = starts.back();
        std::vector<uint8_t> packed((total + 3) / 4 + 16, 0);
        for (size_t r = 0; r < reads.size(); ++r)  // (base by base: any source offset to any destination offset)
            for (uint64_t i = 0; i < reads[r].len; ++i) {
                const uint64_t s = reads[r].offset + i, d = starts[r] + i;
                packed[d >> 2] |= (uint8_t)(((reads[r].data[s >> 2] >> (2 * (s & 3))) & 3u) << (2 * (d & 3)));
            }
        mm_plan_t *plan = nullptr;
        check(mm_plan_create(&plan, k_, w_, CANONICAL, (mm_mode_t)SYNCMER, has_hasher_ ? &hasher_ : nullptr));
        const uint64_t cap = total ? total : 1;
        pos.assign(cap, 0);
        std::vector<uint32_t> sk(sk_ ? cap : 0);
        offsets.assign(reads.size() + 1, 0);
        uint64_t n = 0;
        const int r = mm_run_packed_reads_host(plan, ws.get(), packed.data(), reads.size(), starts.data(), longest, pos.data(),
                                               sk_ ? sk.data() : nullptr, cap, offsets.data(), &n);
        mm_plan_destroy(plan);
        check(r);
        pos.resize(n);
        if (sk_) sk_->assign(sk.begin(), sk.begin() + n);
    }

    // run_many over reads that a device packer left (mm_fastq_pack_device_async / mm_fasta_pack_device_async), their two
    // counts still in DEVICE memory (mm_run_packed_reads_counts_device_async): queued on the workspace's stream behind the
    // packer, nothing waits - Workspace::check_async() (mm_workspace_check) is the one wait, and reports counts beyond the bounds
    // as MM_ERR_CAPACITY.  Device pointers throughout: d_packed / d_read_starts [max_records + 1] / d_counts {bases, records}
    // as the packer wrote them, max_bases / max_records their upper bounds (the text length, the packer's max_records);
    // d_out_offsets [max_records + 1] is written whole (reads past the real count are empty), so
    // mm_values_u64_reads_device_async follows with n_reads = max_records.  With .super_kmers(..) configured pass d_out_sk.
    // The reference has no counterpart: its loader and Builder::run are synchronous (bench/src/lib.rs:51-82, src/lib.rs:378).
    void run_many_counts_device(const void *d_packed, uint64_t packed_bytes, uint64_t max_bases, uint64_t max_records,
                                const uint64_t *d_read_starts, const uint64_t *d_counts, uint32_t *d_out_pos,
                                uint64_t capacity, uint64_t *d_out_offsets, uint64_t *d_count = nullptr,
                                uint32_t *d_out_sk = nullptr) const {
        Workspace &ws = ws_ ? *ws_ : Workspace::thread_default();
        mm_plan_t *plan = nullptr;
        check(mm_plan_create(&plan, k_, w_, CANONICAL, (mm_mode_t)SYNCMER, has_hasher_ ? &hasher_ : nullptr));
        const int r = mm_run_packed_reads_counts_device_async(plan, ws.get(), d_packed, packed_bytes, 0, max_bases, max_records,
                                                              d_read_starts, d_counts, d_out_pos, d_out_sk, capacity,
                                                              d_out_offsets, d_count);
        mm_plan_destroy(plan);
        check(r);
    }

    // A FASTA / FASTQ source of ANY size through the device in chunks (mm_fastx_stream_*): `reader(buf, cap)` fills up to
    // cap bytes and returns how many (0 at the end), `on_batch(const mm_fastx_batch_t &)` receives every batch - the records
    // that lie whole inside one chunk, with absolute 64-bit text offsets; its pointers are valid until on_batch returns.
    // `options`: device and first_byte as given; format, slots, chunk_bytes, max_records, max_positions as given; flags: the
    // MM_FASTX_* bits (super-k-mer indices arrive in the batch, whatever .super_kmers(..) was configured with).  The
    // reference's loader reads any file record by record on the CPU (bench/src/lib.rs:51-82); it has no other counterpart.
    // With MM_FASTX_LONG_RECORDS among the flags a FASTA record longer than a chunk arrives in pieces: an `on_batch` that
    // takes (const mm_fastx_batch_t &, const mm_fastx_pieces_t &) receives mm_fastx_stream_pieces() of every batch with it
    // (fastx_pieces() below for a stream driven by hand).  With MM_FASTX_ONE_MINIMIZER an `on_batch` that takes
    // (const mm_fastx_batch_t &, const uint32_t *one_min) receives the batch's one minimizer per record with it
    // (mm_fastx_stream_one_minimizer: [n_records] words, MM_NO_MINIMIZER for a record without a k-mer - with
    // MM_FASTX_SKIP_AMBIGUOUS without a clean one; nullptr without the flag).
    // `bgzf`: the source is BGZF-compressed (bgzip, htslib) and goes through mm_fastx_stream_feed_bgzf, inflated on the device:
    // 1 yes, 0 no, -1 decided by the source's first bytes (1f 8b 08 with FLG bit 2; such input was MM_ERR_FORMAT before).
    // Plain gzip is refused (MM_ERR_FORMAT).  Offsets in the batches are offsets in the inflated text.
    // MM_FASTX_BGZF_CRC in options.flags: every block's CRC32 is verified on the device; a mismatch throws MM_ERR_FORMAT ("CRC32").
    template <class Reader, class OnBatch>
    void stream_fastx(Reader &&reader, OnBatch &&on_batch, const mm_fastx_stream_config_t &options,
                      size_t read_bytes = size_t(1) << 22, int bgzf = -1) const {
        mm_plan_t *plan = nullptr;
        check(mm_plan_create(&plan, k_, w_, CANONICAL, (mm_mode_t)SYNCMER, has_hasher_ ? &hasher_ : nullptr));
        mm_fastx_stream_t *st = nullptr;
        int r = mm_fastx_stream_create(&st, plan, &options);
        if (r == MM_OK) {
            auto deliver = [&](const mm_fastx_batch_t &b) {
                if constexpr (std::is_invocable_v<OnBatch &, const mm_fastx_batch_t &, const mm_fastx_pieces_t &>)
                    on_batch(b, fastx_pieces(st));
                else if constexpr (std::is_invocable_v<OnBatch &, const mm_fastx_batch_t &, const uint32_t *>)
                    on_batch(b, fastx_one_minimizer(st));
                else
                    on_batch(b);
            };
            r = pump_stream(st, plan, reader, deliver, read_bytes, bgzf);
        }
        mm_plan_destroy(plan);
        check(r);
    }

    // The same for a FASTA of BYTE TEXT (protein; mm_fastx_text_stream_create on this builder's text plan and
    // .text_hasher(..)): `on_batch(const mm_fastx_batch_t &, const mm_fastx_text_extras_t &)` receives every batch with its
    // one minimizer per record (MM_FASTX_TEXT_ONE_MINIMIZER) and the records' bytes (MM_FASTX_TEXT_SEQ); n_bases counts
    // characters, rec_base holds the records' starts.  The reference reads such a file record by record on the CPU
    // (bench/src/lib.rs:51-82) and runs Builder::run on &[u8] per record (src/lib.rs:378).  `bgzf` as stream_fastx takes it.
    template <class Reader, class OnBatch>
    void stream_fasta_text(Reader &&reader, OnBatch &&on_batch, const mm_fastx_text_stream_config_t &options,
                           size_t read_bytes = size_t(1) << 22, int bgzf = -1) const {
        mm_plan_t *plan = nullptr;
        check(mm_plan_create_text(&plan, k_, w_, CANONICAL, (mm_mode_t)SYNCMER, has_text_hasher_ ? &text_hasher_ : nullptr));
        mm_fastx_stream_t *st = nullptr;
        int r = mm_fastx_text_stream_create(&st, plan, &options);
        if (r == MM_OK) {
            auto deliver = [&](const mm_fastx_batch_t &b) {
                mm_fastx_text_extras_t x;
                check(mm_fastx_text_stream_extras(st, &x));
                on_batch(b, x);
            };
            r = pump_stream(st, plan, reader, deliver, read_bytes, bgzf);
        }
        mm_plan_destroy(plan);
        check(r);
    }

    // What the batch last returned by mm_fastx_stream_next says about pieces (mm_fastx_stream_pieces; zeros without
    // MM_FASTX_LONG_RECORDS).
    static mm_fastx_pieces_t fastx_pieces(const mm_fastx_stream_t *st) {
        mm_fastx_pieces_t p;
        check(mm_fastx_stream_pieces(st, &p));
        return p;
    }

    // The one minimizer per record of the batch last returned by mm_fastx_stream_next (mm_fastx_stream_one_minimizer;
    // nullptr without MM_FASTX_ONE_MINIMIZER).
    static const uint32_t *fastx_one_minimizer(const mm_fastx_stream_t *st) {
        const uint32_t *one_min = nullptr;
        uint64_t n = 0;
        check(mm_fastx_stream_one_minimizer(st, &one_min, &n));
        return one_min;
    }

    // Output::values_u64 / values_u128 (src/lib.rs:584-629) of EVERY read of run_many in ONE call (mm_values_u64_reads_host /
    // mm_values_u128_reads_host): `reads`, `pos` and `offsets` as run_many took and wrote them; read r's values are
    // [offsets[r] .. offsets[r + 1]) of the result, what run(reads[r], ..).values_u64() returns.
    std::vector<uint64_t> values_u64_many(const std::vector<PackedSeq> &reads, const std::vector<uint32_t> &pos,
                                          const std::vector<uint64_t> &offsets) const {
        return values_many_raw(reads, pos, offsets, false);
    }
    std::vector<u128> values_u128_many(const std::vector<PackedSeq> &reads, const std::vector<uint32_t> &pos,
                                       const std::vector<uint64_t> &offsets) const {
        const std::vector<uint64_t> raw = values_many_raw(reads, pos, offsets, true);
        std::vector<u128> v(raw.size() / 2);
        for (size_t i = 0; i < v.size(); ++i) v[i] = ((u128)raw[2 * i + 1] << 64) | raw[2 * i];
        return v;
    }

    // run_skip_ambiguous_windows (src/lib.rs:451-496) per read over MANY PackedNSeq reads in ONE call
    // (mm_run_packed_reads_skip_ambiguous_host): codes and ambiguity bits are packed back to back on the host.  Canonical
    // builders only, no super-k-mer indices.  pos / offsets are OVERWRITTEN, read r's read-local positions at
    // pos[offsets[r] .. offsets[r + 1]).
    void run_many_skip_ambiguous_windows(const std::vector<PackedNSeq> &reads, std::vector<uint32_t> &pos,
                                         std::vector<uint64_t> &offsets) const {
        static_assert(CANONICAL, "run_skip_ambiguous_windows() is only defined for canonical builders");
        Workspace &ws = ws_ ? *ws_ : Workspace::thread_default();
        std::vector<uint64_t> starts(reads.size() + 1, 0);
        uint32_t longest = 0;
        for (size_t r = 0; r < reads.size(); ++r) {
            starts[r + 1] = starts[r] + reads[r].seq.len;
            if (reads[r].seq.len > longest) longest = (uint32_t)reads[r].seq.len;
        }
        const uint64_t total = starts.back();
        std::vector<uint8_t> packed((total + 3) / 4 + 16, 0), amb((total + 7) / 8 + 16, 0);
        for (size_t r = 0; r < reads.size(); ++r)
            for (uint64_t i = 0; i < reads[r].seq.len; ++i) {
                const uint64_t s = reads[r].seq.offset + i, a = reads[r].amb_offset + i, d = starts[r] + i;
                packed[d >> 2] |= (uint8_t)(((reads[r].seq.data[s >> 2] >> (2 * (s & 3))) & 3u) << (2 * (d & 3)));
                amb[d >> 3] |= (uint8_t)(((reads[r].amb[a >> 3] >> (a & 7)) & 1u) << (d & 7));
            }
        mm_plan_t *plan = nullptr;
        check(mm_plan_create(&plan, k_, w_, CANONICAL, (mm_mode_t)SYNCMER, has_hasher_ ? &hasher_ : nullptr));
        const uint64_t cap = total ? total : 1;
        pos.assign(cap, 0);
        offsets.assign(reads.size() + 1, 0);
        uint64_t n = 0;
        const int r = mm_run_packed_reads_skip_ambiguous_host(plan, ws.get(), packed.data(), amb.data(), reads.size(),
                                                              starts.data(), longest, pos.data(), cap, offsets.data(), &n);
        mm_plan_destroy(plan);
        check(r);
        pos.resize(n);
    }

    // Builder::run per record over many records of byte text (src/lib.rs:378) in ONE call (mm_run_text_batch_host):
    // pos and offsets are OVERWRITTEN, record r's record-local positions at pos[offsets[r] .. offsets[r + 1]); the
    // super-k-mer indices (super_kmers()) likewise overwrite their vector.
    void run_many(const std::vector<TextSeq> &records, std::vector<uint32_t> &pos, std::vector<uint64_t> &offsets) const {
        Workspace &ws = ws_ ? *ws_ : Workspace::thread_default();
        std::vector<uint64_t> starts(records.size() + 1, 0);
        for (size_t r = 0; r < records.size(); ++r) starts[r + 1] = starts[r] + records[r].len;
        const uint64_t total = starts.back();
        std::vector<uint8_t> text(total ? total : 1);
        for (size_t r = 0; r < records.size(); ++r)
            if (records[r].len) memcpy(text.data() + starts[r], records[r].data, records[r].len);
        mm_plan_t *plan = nullptr;
        check(mm_plan_create_text(&plan, k_, w_, CANONICAL, (mm_mode_t)SYNCMER,
                                  has_text_hasher_ ? &text_hasher_ : nullptr));
        const uint64_t cap = total ? total : 1;
        pos.assign(cap, 0);
        std::vector<uint32_t> sk(sk_ ? cap : 0);
        offsets.assign(records.size() + 1, 0);
        uint64_t n = 0;
        const int r = mm_run_text_batch_host(plan, ws.get(), text.data(), records.size(), starts.data(), pos.data(),
                                             sk_ ? sk.data() : nullptr, cap, offsets.data(), &n);
        mm_plan_destroy(plan);
        check(r);
        pos.resize(n);
        if (sk_) sk_->assign(sk.begin(), sk.begin() + n);
    }

    // Output::values_u64 / values_u128 (src/lib.rs:584-629) of byte text (mm_values_u64_text_host /
    // mm_values_u128_text_host): `pos` as run(TextSeq, ..) wrote them; `encoding` names the Seq the text stands for,
    // MM_TEXT_VALUES_BYTES (`&[u8]`, 8 bits per character, len <= 8 / 16, forward builders only) or MM_TEXT_VALUES_DNA
    // (AsciiSeq, 2 bits per character, len <= 32 / 64).
    std::vector<uint64_t> values_u64(TextSeq seq, const std::vector<uint32_t> &pos, int encoding) const {
        return values_text_raw(seq, pos, encoding, false);
    }
    std::vector<u128> values_u128(TextSeq seq, const std::vector<uint32_t> &pos, int encoding) const {
        return widen(values_text_raw(seq, pos, encoding, true));
    }
    // The same of EVERY record of run_many(records, ..) in ONE call (mm_values_u64_text_batch_host /
    // mm_values_u128_text_batch_host): `pos` and `offsets` as run_many wrote them; record r's values are
    // [offsets[r] .. offsets[r + 1]) of the result, what values_u64(records[r], ..) returns for it alone.
    std::vector<uint64_t> values_u64_many(const std::vector<TextSeq> &records, const std::vector<uint32_t> &pos,
                                          const std::vector<uint64_t> &offsets, int encoding) const {
        return values_text_many_raw(records, pos, offsets, encoding, false);
    }
    std::vector<u128> values_u128_many(const std::vector<TextSeq> &records, const std::vector<uint32_t> &pos,
                                       const std::vector<uint64_t> &offsets, int encoding) const {
        return widen(values_text_many_raw(records, pos, offsets, encoding, true));
    }

    // the immutable plan of this builder (caller destroys it); k and w
    mm_plan_t *make_plan() const {
        mm_plan_t *plan = nullptr;
        check(mm_plan_create(&plan, k_, w_, CANONICAL, (mm_mode_t)SYNCMER, has_hasher_ ? &hasher_ : nullptr));
        return plan;
    }
    uint32_t k() const { return k_; }
    uint32_t w() const { return w_; }

  private:
    // The feed / next loop of both streams; destroys the stream (and, when `deliver` throws, the plan) before it returns.
    template <class Reader, class Deliver>
    // `bgzf` (1 / 0 / -1: by the first four bytes): BGZF blocks go through mm_fastx_stream_feed_bgzf, which takes whole blocks;
    // the front of a block that a read ended in is kept (`held`) and fed again with the bytes that follow.
    static int pump_stream(mm_fastx_stream_t *st, mm_plan_t *plan, Reader &&reader, Deliver &&deliver, size_t read_bytes, int bgzf = 0) {
        int r = MM_OK;
        std::vector<uint8_t> buf(read_bytes ? read_bytes : 1);
        mm_fastx_batch_t batch;
        size_t held = 0;
        // feeds [p, p + n), handing out batches where the stream wants that; returns the bytes taken - all of them, or with
        // BGZF everything in front of an incomplete block: no byte taken twice in a row although mm_fastx_stream_next, which
        // frees the slot of the batch handed out before, wanted input in between
        auto push = [&](const uint8_t *p, size_t n) {
            size_t done = 0;
            bool stalled = false;
            while (done < n && r == MM_OK) {
                uint64_t took = 0;
                r = bgzf > 0 ? mm_fastx_stream_feed_bgzf(st, p + done, n - done, &took) : mm_fastx_stream_feed(st, p + done, n - done, &took);
                done += (size_t)took;
                if (took) stalled = false;
                if (r == MM_OK && done < n) {
                    r = mm_fastx_stream_next(st, &batch);
                    if (r == MM_OK) {
                        deliver(batch);
                    } else if (r == MM_FASTX_NEED_INPUT) {
                        r = MM_OK;
                        if (bgzf > 0 && took == 0) {
                            if (stalled) break;
                            stalled = true;
                        }
                    }
                }
            }
            return done;
        };
        try {
            for (;;) {
                if (held == buf.size()) buf.resize(held + (read_bytes > 65536 ? read_bytes : 65536));
                const size_t got = reader(buf.data() + held, buf.size() - held);
                if (got == 0) break;
                const size_t have = held + got;
                if (bgzf < 0) {
                    if (have < 4) {
                        held = have;
                        continue;
                    }
                    bgzf = buf[0] == 0x1f && buf[1] == 0x8b && buf[2] == 8 && (buf[3] & 4) ? 1 : 0;
                }
                const size_t done = push(buf.data(), have);
                if (r != MM_OK) break;
                held = have - done;
                if (held) memmove(buf.data(), buf.data() + done, held);
            }
            // (a source of fewer than four bytes is text; what is left of a BGZF source is a truncated block, named at finish)
            if (r == MM_OK && held) push(buf.data(), held);
            if (r == MM_OK) r = mm_fastx_stream_finish(st);
            while (r == MM_OK) {
                r = mm_fastx_stream_next(st, &batch);
                if (r == MM_OK) deliver(batch);
            }
            if (r == MM_FASTX_END) r = MM_OK;
        } catch (...) {
            mm_fastx_stream_destroy(st);
            mm_plan_destroy(plan);
            throw;
        }
        mm_fastx_stream_destroy(st);
        return r;
    }

    // one pass of the hot path over `seq` on the device; fills pos (and sk), returns the count
    uint64_t compute(PackedSeq seq, Workspace &ws, std::vector<uint32_t> &pos, std::vector<uint32_t> &sk) const {
        mm_plan_t *plan = nullptr;
        check(mm_plan_create(&plan, k_, w_, CANONICAL, (mm_mode_t)SYNCMER, has_hasher_ ? &hasher_ : nullptr));
        const uint64_t l = (uint64_t)k_ + w_ - 1;
        const uint64_t cap = seq.len >= l ? seq.len - l + 1 : 0;
        pos.assign(cap ? cap : 1, 0);
        sk.assign(sk_ ? (cap ? cap : 1) : 0, 0);
        uint64_t n = 0;
        const int r = mm_run_host(plan, ws.get(), seq.data, seq.offset, seq.len, pos.data(),
                                  sk_ ? sk.data() : nullptr, cap, &n);
        mm_plan_destroy(plan);
        check(r);
        return n;
    }

    std::vector<uint64_t> values_many_raw(const std::vector<PackedSeq> &reads, const std::vector<uint32_t> &pos,
                                          const std::vector<uint64_t> &offsets, bool wide) const {
        if (offsets.size() != reads.size() + 1) throw Error(MM_ERR_NULL);
        Workspace &ws = ws_ ? *ws_ : Workspace::thread_default();
        std::vector<uint64_t> starts(reads.size() + 1, 0);
        for (size_t r = 0; r < reads.size(); ++r) starts[r + 1] = starts[r] + reads[r].len;
        const uint64_t total = starts.back();
        std::vector<uint8_t> packed((total + 3) / 4 + 1, 0);
        for (size_t r = 0; r < reads.size(); ++r)  // (base by base: any source offset to any destination offset)
            for (uint64_t i = 0; i < reads[r].len; ++i) {
                const uint64_t s = reads[r].offset + i, d = starts[r] + i;
                packed[d >> 2] |= (uint8_t)(((reads[r].data[s >> 2] >> (2 * (s & 3))) & 3u) << (2 * (d & 3)));
            }
        const uint64_t n = offsets.back();
        if (pos.size() < n) throw Error(MM_ERR_CAPACITY);
        std::vector<uint64_t> v((wide ? 2 : 1) * n);
        const uint32_t len = SYNCMER ? k_ + w_ - 1 : k_;
        check((wide ? mm_values_u128_reads_host : mm_values_u64_reads_host)(
            ws.get(), packed.data(), packed.size(), 0, reads.size(), starts.data(), 0, len, CANONICAL, pos.data(),
            offsets.data(), v.data()));
        return v;
    }

    static std::vector<u128> widen(const std::vector<uint64_t> &raw) {
        std::vector<u128> v(raw.size() / 2);
        for (size_t i = 0; i < v.size(); ++i) v[i] = ((u128)raw[2 * i + 1] << 64) | raw[2 * i];
        return v;
    }

    std::vector<uint64_t> values_text_raw(TextSeq seq, const std::vector<uint32_t> &pos, int encoding, bool wide) const {
        Workspace &ws = ws_ ? *ws_ : Workspace::thread_default();
        std::vector<uint64_t> v((wide ? 2 : 1) * pos.size());
        const uint32_t len = SYNCMER ? k_ + w_ - 1 : k_;
        check((wide ? mm_values_u128_text_host : mm_values_u64_text_host)(ws.get(), seq.data, seq.len, encoding, len, CANONICAL,
                                                                         pos.data(), pos.size(), v.data()));
        return v;
    }

    std::vector<uint64_t> values_text_many_raw(const std::vector<TextSeq> &records, const std::vector<uint32_t> &pos,
                                               const std::vector<uint64_t> &offsets, int encoding, bool wide) const {
        if (offsets.size() != records.size() + 1) throw Error(MM_ERR_NULL);
        Workspace &ws = ws_ ? *ws_ : Workspace::thread_default();
        std::vector<uint64_t> starts(records.size() + 1, 0);
        for (size_t r = 0; r < records.size(); ++r) starts[r + 1] = starts[r] + records[r].len;
        std::vector<uint8_t> text(starts.back() ? starts.back() : 1);
        for (size_t r = 0; r < records.size(); ++r)
            if (records[r].len) memcpy(text.data() + starts[r], records[r].data, records[r].len);
        const uint64_t n = offsets.back();
        if (pos.size() < n) throw Error(MM_ERR_CAPACITY);
        std::vector<uint64_t> v((wide ? 2 : 1) * n);
        const uint32_t len = SYNCMER ? k_ + w_ - 1 : k_;
        check((wide ? mm_values_u128_text_batch_host : mm_values_u64_text_batch_host)(
            ws.get(), text.data(), records.size(), starts.data(), encoding, len, CANONICAL, pos.data(), offsets.data(), v.data()));
        return v;
    }

    uint32_t k_, w_;
    mm_hasher_t hasher_{};
    bool has_hasher_ = false;
    mm_text_hasher_t text_hasher_{};
    bool has_text_hasher_ = false;
    std::vector<uint32_t> *sk_ = nullptr;
    Workspace *ws_ = nullptr;
};

// Several devices from one call: the reference's rayon loop over contigs (bench/src/bin/paper.rs:442-459) behind
// the C ABI.  A group holds one workspace per listed device (a device may be listed more than once).
class DeviceGroup {
  public:
    explicit DeviceGroup(const std::vector<int> &devices) {
        check(mm_device_group_create(&g_, devices.data(), (int)devices.size()));
    }
    ~DeviceGroup() { mm_device_group_destroy(g_); }
    DeviceGroup(const DeviceGroup &) = delete;
    DeviceGroup &operator=(const DeviceGroup &) = delete;
    mm_device_group_t *get() const { return g_; }
    int size() const { return mm_device_group_size(g_); }

    // Builder::run over all devices of the group: one sequence cut into window ranges (absolute positions,
    // exact seam); positions are APPENDED to min_pos with the last() rule like run()
    template <bool CANONICAL, int SYNCMER>
    void run(const Builder<CANONICAL, SYNCMER> &b, PackedSeq seq, std::vector<uint32_t> &min_pos) const {
        mm_plan_t *plan = b.make_plan();
        const uint64_t l = (uint64_t)b.k() + b.w() - 1;
        const uint64_t cap = seq.len >= l ? seq.len - l + 1 : 0;
        std::vector<uint32_t> pos(cap ? cap : 1);
        uint64_t n = 0;
        const int r = mm_run_sharded_host(plan, g_, seq.data, seq.offset, seq.len, pos.data(), nullptr, cap, &n);
        mm_plan_destroy(plan);
        check(r);
        size_t first = 0;
        if (SYNCMER == 0)
            while (first < n && !min_pos.empty() && pos[first] == min_pos.back()) ++first;
        min_pos.insert(min_pos.end(), pos.begin() + first, pos.begin() + n);
    }
    // one Builder::run per sequence (paper.rs:425-431), the sequences placed greedily on the devices: positions
    // are sequence-local, sequence s = pos[offsets[s] .. offsets[s + 1])
    template <bool CANONICAL, int SYNCMER>
    void run_batch(const Builder<CANONICAL, SYNCMER> &b, const std::vector<PackedSeq> &seqs, std::vector<uint32_t> &pos,
                   std::vector<uint64_t> &offsets) const {
        mm_plan_t *plan = b.make_plan();
        std::vector<const uint8_t *> ptr;
        std::vector<uint64_t> off, len;
        uint64_t cap = 1;
        for (const PackedSeq &s : seqs) {
            ptr.push_back(s.data);
            off.push_back(s.offset);
            len.push_back(s.len);
            cap += s.len;
        }
        pos.assign(cap, 0);
        offsets.assign(seqs.size() + 1, 0);
        const int r = mm_run_batch_sharded_host(plan, g_, seqs.size(), ptr.data(), off.data(), len.data(), pos.data(),
                                                nullptr, cap, offsets.data());
        mm_plan_destroy(plan);
        check(r);
        pos.resize(offsets.back());
    }

    // ---- device-resident shards (round 4): the sequence lives in HBM on every device of the group, every device
    // walks its window range with one asynchronous launch, the positions stay where they were made
    void upload(PackedSeq seq) { check(mm_device_group_upload(g_, seq.data, (seq.offset + seq.len + 3) / 4)); }
    /// Every device receives only what its share of an N-way split of `seq` reads (one crossing of the host link in total).
    void upload_shares(PackedSeq seq) {
        check(mm_device_group_upload_range(g_, seq.data, (seq.offset + seq.len + 3) / 4, seq.offset, seq.len));
    }
    void adopt(const std::vector<const void *> &d_packed, uint64_t packed_bytes) {
        check(mm_device_group_adopt(g_, d_packed.data(), packed_bytes));
    }
    // per-entry counts of Builder::run over the resident sequence (n_bases bases from base_offset on)
    template <bool CANONICAL, int SYNCMER>
    std::vector<uint64_t> run_device(const Builder<CANONICAL, SYNCMER> &b, uint64_t n_bases, uint64_t base_offset = 0,
                                     bool super_kmers = false) const {
        mm_plan_t *plan = b.make_plan();
        std::vector<uint64_t> counts((size_t)size());
        const int r = mm_run_sharded_device(plan, g_, base_offset, n_bases, super_kmers ? 1 : 0, counts.data(), nullptr);
        mm_plan_destroy(plan);
        check(r);
        return counts;
    }
    struct Shard {
        uint32_t *d_pos = nullptr, *d_sk = nullptr;  // device pointers on the entry's device
        uint64_t count = 0, win_begin = 0, win_end = 0;
    };
    Shard result(int entry) const {
        Shard s;
        check(mm_device_group_result(g_, entry, &s.d_pos, &s.d_sk, &s.count, &s.win_begin, &s.win_end));
        return s;
    }
    // device-resident BATCHES: independent sequences placed greedily on the entries, each on its entry's device only;
    // one batch launch per entry; sequence-local positions stay on the devices (mm_device_group_batch_result)
    void upload_batch(const std::vector<PackedSeq> &seqs) {
        std::vector<const uint8_t *> ptr;
        std::vector<uint64_t> bytes;
        for (const PackedSeq &s : seqs) {
            ptr.push_back(s.data);
            bytes.push_back((s.offset + s.len + 3) / 4);
        }
        check(mm_device_group_upload_batch(g_, seqs.size(), ptr.data(), bytes.data()));
    }
    template <bool CANONICAL, int SYNCMER>
    std::vector<uint64_t> run_batch_device(const Builder<CANONICAL, SYNCMER> &b, const std::vector<PackedSeq> &seqs) const {
        mm_plan_t *plan = b.make_plan();
        std::vector<uint64_t> off, len, counts(seqs.size());
        for (const PackedSeq &s : seqs) {
            off.push_back(s.offset);
            len.push_back(s.len);
        }
        const int r = mm_run_batch_sharded_device(plan, g_, off.data(), len.data(), 0, counts.data(), nullptr);
        mm_plan_destroy(plan);
        check(r);
        return counts;
    }
    // Output::values_u64 / values_u128 (src/lib.rs:584-629) of the last run_batch_device's positions, every entry's
    // sequences in ONE launch (mm_device_group_values_batch); the values stay on the devices.  Returns their number.
    template <bool CANONICAL, int SYNCMER>
    uint64_t values_batch(const Builder<CANONICAL, SYNCMER> &b, bool u128 = false) const {
        const uint32_t len = SYNCMER ? b.k() + b.w() - 1 : b.k();
        uint64_t total = 0;
        check(mm_device_group_values_batch(g_, len, CANONICAL ? 1 : 0, u128 ? 1 : 0, &total));
        return total;
    }
    struct BatchValues {
        int entry = 0;                 // the entry whose device holds them
        uint64_t *d_values = nullptr;  // device pointer: count words, 2 * count ({lo, hi}) after values_batch(b, true)
        uint64_t count = 0;
    };
    // where sequence `seq`'s values lie, until the next upload or run on the group
    BatchValues batch_values(uint64_t seq) const {
        BatchValues v;
        check(mm_device_group_batch_values(g_, seq, &v.entry, &v.d_values, &v.count));
        return v;
    }
    // all sequences, input order, into device memory of entry `root`; returns the n + 1 offsets
    std::vector<uint64_t> gather_batch(int root, size_t n_seqs, uint32_t *d_dst_pos, uint64_t capacity) const {
        std::vector<uint64_t> offs(n_seqs + 1);
        check(mm_device_group_gather_batch(g_, root, d_dst_pos, nullptr, capacity, offs.data()));
        return offs;
    }
    // the shards, dense and in window order, into device memory of entry `root` (device-to-device copies)
    uint64_t gather(int root, uint32_t *d_dst_pos, uint64_t capacity, uint32_t *d_dst_sk = nullptr) const {
        uint64_t total = 0;
        check(mm_device_group_gather(g_, root, d_dst_pos, d_dst_sk, capacity, &total));
        return total;
    }

  private:
    mm_device_group_t *g_ = nullptr;
};

// ---- one_minimizer(seq, hasher) (src/minimizers.rs:22-28, re-exported at src/lib.rs:211): the leftmost position that
// minimises hash & 0xffff0000 over the k-mers of a sequence; no strand vote (the reference has no one_canonical_minimizer,
// FIXME at src/minimizers.rs:30).  `Hasher` is any of the hasher structs above (its `tables` go to the C call).  The
// *_many forms take every record in ONE call (mm_one_minimizer_reads_host / mm_one_minimizer_text_batch_host) and give
// MM_NO_MINIMIZER for a record shorter than k; the single forms throw Error(MM_ERR_CAPACITY) there,
// where the reference's unwrap() panics.
inline std::vector<uint32_t> one_minimizer_many(const std::vector<PackedSeq> &reads, const mm_hasher_t &hasher, uint32_t k,
                                                Workspace *ws = nullptr) {
    Workspace &w = ws ? *ws : Workspace::thread_default();
    std::vector<uint64_t> starts(reads.size() + 1, 0);
    for (size_t r = 0; r < reads.size(); ++r) starts[r + 1] = starts[r] + reads[r].len;
    std::vector<uint8_t> packed((starts.back() + 3) / 4 + 1, 0);
    for (size_t r = 0; r < reads.size(); ++r)  // (base by base: any source offset to any destination offset)
        for (uint64_t i = 0; i < reads[r].len; ++i) {
            const uint64_t s = reads[r].offset + i, d = starts[r] + i;
            packed[d >> 2] |= (uint8_t)(((reads[r].data[s >> 2] >> (2 * (s & 3))) & 3u) << (2 * (d & 3)));
        }
    std::vector<uint32_t> out(reads.size());
    check(mm_one_minimizer_reads_host(w.get(), &hasher, k, packed.data(), packed.size(), 0, reads.size(), starts.data(), 0, 0,
                                      out.data()));
    return out;
}
inline std::vector<uint32_t> one_minimizer_many(const std::vector<TextSeq> &records, const mm_text_hasher_t &hasher, uint32_t k,
                                                Workspace *ws = nullptr) {
    Workspace &w = ws ? *ws : Workspace::thread_default();
    std::vector<uint64_t> starts(records.size() + 1, 0);
    for (size_t r = 0; r < records.size(); ++r) starts[r + 1] = starts[r] + records[r].len;
    std::vector<uint8_t> text(starts.back() + 1, 0);
    for (size_t r = 0; r < records.size(); ++r)
        if (records[r].len) std::memcpy(text.data() + starts[r], records[r].data, records[r].len);
    std::vector<uint32_t> out(records.size());
    check(mm_one_minimizer_text_batch_host(w.get(), &hasher, k, text.data(), starts.back(), records.size(), starts.data(),
                                           out.data()));
    return out;
}
// Reads with ambiguity bits (PackedNSeq): only k-mers without an ambiguous base count, MM_NO_MINIMIZER for a read without one
// (mm_one_minimizer_reads_skip_ambiguous_host: k-mer-level skipping; the reference's one_minimizer takes a plain Seq and
// has no counterpart).  The reads are laid back to back with their bits.
inline std::vector<uint32_t> one_minimizer_many(const std::vector<PackedNSeq> &reads, const mm_hasher_t &hasher, uint32_t k,
                                                Workspace *ws = nullptr) {
    Workspace &w = ws ? *ws : Workspace::thread_default();
    std::vector<uint64_t> starts(reads.size() + 1, 0);
    for (size_t r = 0; r < reads.size(); ++r) starts[r + 1] = starts[r] + reads[r].seq.len;
    std::vector<uint8_t> packed((starts.back() + 3) / 4 + 1, 0), amb((starts.back() + 7) / 8 + 1, 0);
    for (size_t r = 0; r < reads.size(); ++r)
        for (uint64_t i = 0; i < reads[r].seq.len; ++i) {
            const uint64_t s = reads[r].seq.offset + i, a = reads[r].amb_offset + i, d = starts[r] + i;
            packed[d >> 2] |= (uint8_t)(((reads[r].seq.data[s >> 2] >> (2 * (s & 3))) & 3u) << (2 * (d & 3)));
            amb[d >> 3] |= (uint8_t)(((reads[r].amb[a >> 3] >> (a & 7)) & 1u) << (d & 7));
        }
    std::vector<uint32_t> out(reads.size());
    check(mm_one_minimizer_reads_skip_ambiguous_host(w.get(), &hasher, k, packed.data(), packed.size(), 0, amb.data(), amb.size(),
                                                     0, reads.size(), starts.data(), 0, 0, out.data()));
    return out;
}
// The *_many_counts_device forms: records already on the device with their two counts {symbols, records} in DEVICE memory,
// as a loader wrote them (mm_one_minimizer_text_batch_counts_device_async / mm_one_minimizer_reads_counts_device_async):
// asynchronous on `ws`, d_out_pos[0 .. n) filled, MM_NO_MINIMIZER up to max_records; mm_workspace_check reports counts
// beyond the bounds as MM_ERR_CAPACITY.  The reference has no counterpart (one_minimizer is synchronous host code).
inline void one_minimizer_many_counts_device(const mm_text_hasher_t &hasher, uint32_t k, const void *d_text, uint64_t text_bytes,
                                             uint64_t max_chars, uint64_t max_records, const uint64_t *d_starts,
                                             const uint64_t *d_counts, uint32_t *d_out_pos, Workspace *ws = nullptr) {
    Workspace &w = ws ? *ws : Workspace::thread_default();
    check(mm_one_minimizer_text_batch_counts_device_async(w.get(), &hasher, k, d_text, text_bytes, max_chars, max_records,
                                                          d_starts, d_counts, d_out_pos));
}
inline void one_minimizer_many_counts_device(const mm_hasher_t &hasher, uint32_t k, const void *d_packed, uint64_t packed_bytes,
                                             uint64_t base_offset, uint64_t max_bases, uint64_t max_records,
                                             const uint64_t *d_read_starts, const uint64_t *d_counts, uint32_t *d_out_pos,
                                             Workspace *ws = nullptr) {
    Workspace &w = ws ? *ws : Workspace::thread_default();
    check(mm_one_minimizer_reads_counts_device_async(w.get(), &hasher, k, d_packed, packed_bytes, base_offset, max_bases,
                                                     max_records, d_read_starts, d_counts, d_out_pos));
}
// (the packed form over the N packers' ambiguity bits: mm_one_minimizer_reads_skip_ambiguous_counts_device_async)
inline void one_minimizer_many_counts_device(const mm_hasher_t &hasher, uint32_t k, const void *d_packed, uint64_t packed_bytes,
                                             uint64_t base_offset, const void *d_amb, uint64_t amb_bytes, uint64_t amb_offset,
                                             uint64_t max_bases, uint64_t max_records, const uint64_t *d_read_starts,
                                             const uint64_t *d_counts, uint32_t *d_out_pos, Workspace *ws = nullptr) {
    Workspace &w = ws ? *ws : Workspace::thread_default();
    check(mm_one_minimizer_reads_skip_ambiguous_counts_device_async(w.get(), &hasher, k, d_packed, packed_bytes, base_offset,
                                                                    d_amb, amb_bytes, amb_offset, max_bases, max_records,
                                                                    d_read_starts, d_counts, d_out_pos));
}
template <class Hasher>
inline std::vector<uint32_t> one_minimizer_many(const std::vector<PackedNSeq> &reads, const Hasher &hasher, uint32_t k) {
    return one_minimizer_many(reads, hasher.tables, k);
}
// (MM_NO_MINIMIZER when the read has no clean k-mer; Error(MM_ERR_CAPACITY) when it is shorter than k, as the plain form)
template <class Hasher>
inline uint32_t one_minimizer(PackedNSeq seq, const Hasher &hasher, uint32_t k) {
    if (seq.seq.len < k) throw Error(MM_ERR_CAPACITY);
    return one_minimizer_many(std::vector<PackedNSeq>{seq}, hasher.tables, k)[0];
}
template <class Hasher>
inline std::vector<uint32_t> one_minimizer_many(const std::vector<PackedSeq> &reads, const Hasher &hasher, uint32_t k) {
    return one_minimizer_many(reads, hasher.tables, k);
}
template <class Hasher>
inline std::vector<uint32_t> one_minimizer_many(const std::vector<TextSeq> &records, const Hasher &hasher, uint32_t k) {
    return one_minimizer_many(records, hasher.tables, k);
}
template <class Hasher>
inline uint32_t one_minimizer(PackedSeq seq, const Hasher &hasher, uint32_t k) {
    if (seq.len < k) throw Error(MM_ERR_CAPACITY);
    return one_minimizer_many(std::vector<PackedSeq>{seq}, hasher.tables, k)[0];
}
template <class Hasher>
inline uint32_t one_minimizer(TextSeq seq, const Hasher &hasher, uint32_t k) {
    if (seq.len < k) throw Error(MM_ERR_CAPACITY);
    return one_minimizer_many(std::vector<TextSeq>{seq}, hasher.tables, k)[0];
}

// constructors, src/lib.rs:240-321
inline Builder<false, 0> minimizers(uint32_t k, uint32_t w) { return {k, w}; }
inline Builder<true, 0> canonical_minimizers(uint32_t k, uint32_t w) { return {k, w}; }
inline Builder<false, 1> closed_syncmers(uint32_t k, uint32_t w) { return {k, w}; }
inline Builder<true, 1> canonical_closed_syncmers(uint32_t k, uint32_t w) { return {k, w}; }
inline Builder<false, 2> open_syncmers(uint32_t k, uint32_t w) { return {k, w}; }
inline Builder<true, 2> canonical_open_syncmers(uint32_t k, uint32_t w) { return {k, w}; }
inline Builder<true, 1> canonical_syncmers(uint32_t k, uint32_t w) { return {k, w}; }  // README.md:65 name

// free functions, src/lib.rs:639-654
inline std::vector<uint32_t> minimizer_positions(PackedSeq s, uint32_t k, uint32_t w) { return minimizers(k, w).run_once(s); }
inline std::vector<uint32_t> minimizer_positions(AsciiSeq s, uint32_t k, uint32_t w) { return minimizers(k, w).run_once(s); }
inline std::vector<uint32_t> canonical_minimizer_positions(PackedSeq s, uint32_t k, uint32_t w) {
    return canonical_minimizers(k, w).run_once(s);
}

}  // namespace simd_minimizers
