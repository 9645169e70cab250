// The C++ mirror of the builder on &[u8] text (src/lib.rs:59): Builder::run(TextSeq, pos) and .hasher(text tables).
// Exit code 0 = all checks passed; 77 = no GPU (the engine has no CPU fallback).
#include <cstdio>
#include <cstring>
#include <random>

#include "simd_minimizers_amd.hpp"

using namespace simd_minimizers;

int main() {
    if (mm_device_count() <= 0) return 77;
    // the AsciiSeq doctest (src/lib.rs:92-101) as byte text with NtHasher's tables over ASCII DNA
    mm_text_hasher_t dna;
    const NtHasher<false> nt(5);
    check(mm_text_hasher_from_dna(&dna, &nt.tables));
    const char *seq = "ACGTGCTCAGAGACTCAG";
    const TextSeq t{(const uint8_t *)seq, strlen(seq)};
    if (minimizers(5, 7).hasher(dna).run_once(t) != std::vector<uint32_t>{4, 5, 8, 13}) return 2;

    // random ASCII DNA: the text path with the DNA table equals the AsciiSeq path, super-k-mer indices included
    std::mt19937 rng(1);
    std::vector<uint8_t> text(100000);
    for (auto &c : text) c = (uint8_t)"ACGTacgt"[rng() & 7];
    std::vector<uint32_t> pos, sk;
    minimizers(21, 11).hasher(dna).super_kmers(&sk).run(TextSeq{text.data(), text.size()}, pos);
    if (pos != minimizers(21, 11).run_once(AsciiSeq{text.data(), text.size()})) return 3;
    if (sk.size() != pos.size() || sk.empty()) return 4;

    // arbitrary bytes with the default MulHasher: appending twice keeps the last() rule; canonical plans build
    for (auto &c : text) c = (uint8_t)rng();
    const TextSeq b{text.data(), text.size()};
    std::vector<uint32_t> a1 = minimizers(21, 11).run_once(b), a2;
    if (a1.empty()) return 5;
    minimizers(21, 11).hasher(TextMulHasher<false>(21)).run(b, a2);
    if (a1 != a2) return 6;
    if (canonical_minimizers(21, 11).run_once(b).empty()) return 7;

    // a text plan is refused by the packed entry points
    mm_plan_t *plan = nullptr;
    check(mm_plan_create_text(&plan, 5, 7, 0, MM_MINIMIZERS, nullptr));
    uint64_t n = 0;
    const int r = mm_run_host(plan, Workspace::thread_default().get(), text.data(), 0, 100, nullptr, nullptr, 0, &n);
    mm_plan_destroy(plan);
    if (r != MM_ERR_BAD_MODE) return 8;
    printf("text example ok\n");
    return 0;
}
