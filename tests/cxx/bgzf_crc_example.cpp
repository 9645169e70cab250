/* The CRC32 of BGZF blocks, verified on the device on request: mm_bgzf_scan_crc_host hands out the trailers' CRC32s,
 * mm_bgzf_inflate_verify_host inflates a whole file and checks every block, and Builder::stream_fastx with MM_FASTX_BGZF_CRC
 * in options.flags delivers what it delivers without the flag - and throws on a file in which one text byte of a stored block
 * was changed, which the inflate alone takes for text (its structure and ISIZE are still right).  The reference's loader
 * checks the CRC32 inside its decompressor on the CPU (needletail::parse_fastx_file, bench/src/lib.rs:51-82).
 * The BGZF writer below needs no zlib: blocks alternate between stored deflate blocks and fixed-Huffman blocks of literals.
 * Exit code 0 = everything agrees; 77 = no GPU (the engine has no CPU fallback). */
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "simd_minimizers_amd.hpp"

namespace sm = simd_minimizers;

enum { N_READS = 600, K = 21, W = 11 };

struct Collected {
    std::vector<uint64_t> rec_text_pos, offsets{0};
    std::vector<uint32_t> pos;
    uint64_t covered = 0;
    void add(const mm_fastx_batch_t &b) {
        covered = b.text_end;
        for (uint64_t r = 0; r < b.n_records; ++r) {
            rec_text_pos.push_back(b.rec_text_pos[r]);
            offsets.push_back(pos.size() + b.offsets[r + 1]);
        }
        pos.insert(pos.end(), b.pos, b.pos + b.n_positions);
    }
};

static uint32_t crc32_of(const uint8_t *p, size_t n) { /* bit by bit: independent of the library's tables */
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int j = 0; j < 8; ++j) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
    }
    return ~c;
}

struct Bits {
    std::vector<uint8_t> out;
    uint32_t acc = 0, n = 0;
    void put(uint32_t v, uint32_t k) { /* least significant bit first */
        acc |= v << n;
        n += k;
        while (n >= 8) out.push_back((uint8_t)acc), acc >>= 8, n -= 8;
    }
    void code(uint32_t c, uint32_t k) { /* a Huffman code: most significant bit first */
        for (uint32_t i = k; i-- > 0;) put((c >> i) & 1u, 1);
    }
    void flush() {
        if (n) put(0, 8 - n);
    }
};

/* one BGZF block of text[0 .. n), n < 65536; returns the offset of its payload in the file */
static size_t bgzf_block(std::vector<uint8_t> &file, const uint8_t *text, uint32_t n, bool fixed) {
    Bits b;
    if (fixed) {
        b.put(1, 1), b.put(1, 2);
        for (uint32_t i = 0; i < n; ++i) {
            if (text[i] < 144) b.code(0x30 + text[i], 8);
            else b.code(0x190 + (text[i] - 144), 9);
        }
        b.code(0, 7);
        b.flush();
    } else {
        b.put(1, 1), b.put(0, 2), b.flush();
        b.put(n, 16), b.put(n ^ 0xffffu, 16);
        b.out.insert(b.out.end(), text, text + n);
    }
    const uint32_t bsize = 18 + (uint32_t)b.out.size() + 8 - 1, crc = crc32_of(text, n);
    const uint8_t head[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)bsize, (uint8_t)(bsize >> 8)};
    file.insert(file.end(), head, head + 18);
    const size_t payload = file.size();
    file.insert(file.end(), b.out.begin(), b.out.end());
    for (int i = 0; i < 4; ++i) file.push_back((uint8_t)(crc >> (8 * i)));
    for (int i = 0; i < 4; ++i) file.push_back((uint8_t)(n >> (8 * i)));
    return payload;
}

int main() {
    if (mm_device_count() <= 0) {
        printf("no GPU\n");
        return 77;
    }
    std::string text;
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (int r = 0; r < N_READS; ++r) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        const uint64_t len = 50 + (x >> 40) % 250;
        text += "@read" + std::to_string(r) + "\n";
        for (uint64_t j = 0; j < len; ++j) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            text.push_back("ACGT"[(x >> 33) & 3]);
        }
        text += "\n+\n" + std::string(len, 'I') + "\n";
    }
    std::vector<uint8_t> file;
    std::vector<uint32_t> want_crc;
    uint32_t n_blocks = 0;
    size_t flip_at = 0; /* file offset of a base in a stored block far behind the stream's first chunks */
    for (size_t at = 0; at < text.size(); ++n_blocks) {
        const uint32_t n = (uint32_t)(text.size() - at < 3000 + 37 * (n_blocks % 11) ? text.size() - at : 3000 + 37 * (n_blocks % 11));
        const size_t payload = bgzf_block(file, (const uint8_t *)text.data() + at, n, n_blocks % 2 == 1);
        want_crc.push_back(crc32_of((const uint8_t *)text.data() + at, n));
        if (n_blocks == 20) { /* a stored block: 5 bytes of block header, then the text; the first base of a sequence line in it */
            size_t line = text.find("\n@read", at);
            line = text.find('\n', line + 1) + 1;
            if (line <= at || line >= at + n) return 1;
            flip_at = payload + 5 + (line - at);
        }
        at += n;
    }
    bgzf_block(file, nullptr, 0, true); /* the EOF marker's kind: a block without text (its trailer is not checked) */
    if (n_blocks < 30) return 1;

    /* the C ABI: the table and the trailers' CRC32s from the headers; the host function gives the same values */
    std::vector<mm_bgzf_block_t> table(n_blocks + 1);
    std::vector<uint32_t> crcs(n_blocks + 1);
    uint64_t listed = 0, consumed = 0, out_bytes = 0;
    if (mm_bgzf_scan_crc_host(file.data(), file.size(), table.size(), ~0ull, table.data(), &listed, &consumed, &out_bytes, crcs.data()) != MM_OK) {
        printf("scan: %s\n", mm_last_error());
        return 2;
    }
    if (listed != n_blocks || consumed != file.size() || out_bytes != text.size()) return 3;
    for (uint32_t i = 0; i < n_blocks; ++i) {
        uint32_t c = 0;
        if (crcs[i] != want_crc[i]) return 4;
        if (mm_debug_crc32((const uint8_t *)text.data() + table[i].out_off, table[i].isize, &c) != MM_OK || c != want_crc[i]) return 5;
    }

    /* the whole file, inflated and verified on the device; then with one base of a stored block changed */
    mm_workspace_t *ws = nullptr;
    if (mm_workspace_create(&ws, 0, nullptr) != MM_OK) return 6;
    std::vector<uint8_t> back(text.size());
    uint64_t got_bytes = 0;
    if (mm_bgzf_inflate_verify_host(ws, file.data(), file.size(), back.data(), back.size(), &got_bytes) != MM_OK) {
        printf("inflate + verify: %s\n", mm_last_error());
        return 7;
    }
    if (got_bytes != text.size() || memcmp(back.data(), text.data(), text.size()) != 0) return 8;
    std::vector<uint8_t> corrupt(file);
    corrupt[flip_at] = corrupt[flip_at] == 'A' ? 'C' : 'A';
    if (mm_bgzf_inflate_host(ws, corrupt.data(), corrupt.size(), back.data(), back.size(), &got_bytes) != MM_OK) return 9;
    if (memcmp(back.data(), text.data(), text.size()) == 0) return 10; /* (the inflate alone hands out the wrong text) */
    if (mm_bgzf_inflate_verify_host(ws, corrupt.data(), corrupt.size(), back.data(), back.size(), &got_bytes) != MM_ERR_FORMAT) return 11;
    if (!strstr(mm_last_error(), "CRC32")) return 12;
    if (mm_workspace_check(ws) != MM_OK) return 13;
    mm_workspace_destroy(ws);

    /* the stream: without the flag, with it, and with it over the corrupt file */
    mm_fastx_stream_config_t cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.format = MM_FASTX_AUTO;
    cfg.chunk_bytes = 16384;
    cfg.max_records = 1000;
    const auto run = [&](const std::vector<uint8_t> &data, uint32_t flags, Collected &got) {
        size_t at = 0;
        mm_fastx_stream_config_t c = cfg;
        c.flags = flags;
        sm::canonical_minimizers(K, W).stream_fastx(
            [&](uint8_t *buf, size_t cap) {
                const size_t m = data.size() - at < cap ? data.size() - at : cap;
                memcpy(buf, data.data() + at, m);
                at += m;
                return m;
            },
            [&](const mm_fastx_batch_t &b) { got.add(b); }, c, 7001, -1);
    };
    Collected plain, checked, unchecked, failed;
    run(file, 0, plain);
    run(file, MM_FASTX_BGZF_CRC, checked);
    if (plain.rec_text_pos.size() != N_READS || plain.covered != text.size()) return 20;
    if (checked.rec_text_pos != plain.rec_text_pos || checked.offsets != plain.offsets || checked.pos != plain.pos) return 21;
    run(corrupt, 0, unchecked); /* (a base became another base: still a FASTQ, and nobody notices) */
    if (unchecked.rec_text_pos != plain.rec_text_pos) return 22;
    try {
        run(corrupt, MM_FASTX_BGZF_CRC, failed);
        return 23;
    } catch (const sm::Error &e) {
        if (e.code != MM_ERR_FORMAT || !strstr(e.what(), "CRC32")) return 24;
    }
    if (failed.covered > table[20].out_off) return 25; /* (nothing made of the corrupt block's chunk was delivered) */
    printf("bgzf_crc_example: OK (%d reads, %u blocks, %llu bytes of text, %llu positions)\n", (int)N_READS, n_blocks,
           (unsigned long long)text.size(), (unsigned long long)plain.pos.size());
    return 0;
}
