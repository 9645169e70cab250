// A protein FASTA file -> the byte-text stream -> per record: minimizer positions, their k-mer values, one minimizer
// (Builder::stream_fasta_text over mm_fastx_text_stream_create).  The first batch is checked against the one-shot calls
// on its own records (Builder::run_many / values_u64_many on TextSeq, one_minimizer_many), every batch against the file:
// the records' bytes, their headers' offsets, and that the batches tile the file.  Compiling needs no device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "simd_minimizers_amd.hpp"

namespace sm = simd_minimizers;

#define REQUIRE(cond)                                                         \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            return 1;                                                         \
        }                                                                     \
    } while (0)

static uint64_t g_x = 0x2545F4914F6CDD1Dull;
static uint64_t rnd() {
    g_x ^= g_x << 13, g_x ^= g_x >> 7, g_x ^= g_x << 17;
    return g_x;
}

int main() {
    const uint32_t k = 7, w = 11;
    const char letters[] = "ACDEFGHIKLMNPQRSTVWY";
    // the file: 400 records of 0 .. 900 residues in lines of 60
    std::string file;
    std::vector<std::string> seqs;
    std::vector<uint64_t> where;
    for (int r = 0; r < 400; ++r) {
        std::string s(r % 9 == 0 ? r % 5 : rnd() % 901, 'A');
        for (auto &c : s) c = letters[rnd() % 20];
        where.push_back(file.size());
        file += ">sp|P" + std::to_string(r) + "|PROT_" + std::to_string(r) + " example\n";
        for (size_t q = 0; q < s.size(); q += 60) file += s.substr(q, 60) + "\n";
        seqs.push_back(s);
    }
    std::FILE *f = std::tmpfile();
    REQUIRE(f != nullptr);
    REQUIRE(std::fwrite(file.data(), 1, file.size(), f) == file.size());
    std::rewind(f);

    const sm::TextMulHasher<false> hasher(k);
    const auto builder = sm::minimizers(k, w).hasher(hasher);
    mm_fastx_text_stream_config_t cfg{};
    cfg.format = MM_FASTX_AUTO;
    cfg.flags = MM_FASTX_VALUES_U64 | MM_FASTX_TEXT_ONE_MINIMIZER | MM_FASTX_TEXT_SEQ;
    cfg.chunk_bytes = 16384;
    cfg.max_records = 1024;
    cfg.values_encoding = MM_TEXT_VALUES_BYTES;

    size_t record = 0, batches = 0;
    uint64_t at = 0;
    int bad = 0;
    builder.stream_fasta_text(
        [&](uint8_t *buf, size_t cap) { return std::fread(buf, 1, cap < 5000 ? cap : 5000, f); },
        [&](const mm_fastx_batch_t &b, const mm_fastx_text_extras_t &x) {
            if (b.text_begin != at || !x.one_min || !x.seq || !b.values) bad |= 1;
            at = b.text_end;
            std::vector<sm::TextSeq> records;
            for (uint64_t r = 0; r < b.n_records; ++r, ++record) {
                const uint64_t len = b.rec_base[r + 1] - b.rec_base[r];
                if (record >= seqs.size() || b.rec_text_pos[r] != where[record] || len != seqs[record].size() ||
                    std::memcmp(x.seq + b.rec_base[r], seqs[record].data(), len) != 0)
                    bad |= 2;
                records.push_back({x.seq + b.rec_base[r], len});
            }
            if (batches++ == 0) {  // the one-shot calls on the first batch's records
                std::vector<uint32_t> pos;
                std::vector<uint64_t> offsets;
                builder.run_many(records, pos, offsets);
                const std::vector<uint64_t> values = builder.values_u64_many(records, pos, offsets, MM_TEXT_VALUES_BYTES);
                const std::vector<uint32_t> one = sm::one_minimizer_many(records, hasher, k);
                if (offsets.size() != b.n_records + 1 || offsets.back() != b.n_positions || pos.size() < b.n_positions) {
                    bad |= 4;
                } else {
                    if (std::memcmp(offsets.data(), b.offsets, offsets.size() * 8) != 0) bad |= 8;
                    if (std::memcmp(pos.data(), b.pos, b.n_positions * 4) != 0) bad |= 16;
                    if (std::memcmp(values.data(), b.values, b.n_positions * 8) != 0) bad |= 32;
                    if (std::memcmp(one.data(), x.one_min, b.n_records * 4) != 0) bad |= 64;
                }
                for (uint64_t r = 0; r < b.n_records; ++r)
                    if ((records[r].len < k) != (x.one_min[r] == MM_NO_MINIMIZER)) bad |= 128;
            }
        },
        cfg);
    std::fclose(f);
    REQUIRE(bad == 0);
    REQUIRE(record == seqs.size());
    REQUIRE(at == file.size());
    REQUIRE(batches >= 5);
    std::printf("fastx_text_stream_example: %zu records in %zu batches ok\n", record, batches);
    return 0;
}
