// Host threads through the C++ mirror: 8 std::threads share ONE Builder and each uses Workspace::thread_default() (the
// reference's thread-local CACHE, src/lib.rs:217-219).  tests/test_gpu_threads.py writes every thread's inputs to files
// and compares the outputs this program writes with the oracle.
//
//   threads_example DIR N_THREADS
//   DIR/in_T_packed.bin   2-bit packed bases (PackedSeq) of thread T     -> DIR/out_T_run.bin   (uint32 positions)
//   DIR/in_T_nseq.bin     packed bases, DIR/in_T_amb.bin ambiguity bits  -> DIR/out_T_skip.bin  (skip-ambiguous windows)
//   DIR/in_T_text.bin     byte text (TextSeq)                            -> DIR/out_T_text.bin  (uint32 positions)
//   DIR/in_T_len.txt      "n_packed n_nseq"
// Exit code 0 = every thread finished; 77 = no GPU (the engine has no CPU fallback).
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <thread>
#include <vector>

#include "simd_minimizers_amd.hpp"

using namespace simd_minimizers;

static std::vector<uint8_t> read_file(const std::string &path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

static bool write_file(const std::string &path, const std::vector<uint32_t> &v) {
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char *>(v.data()), (std::streamsize)(v.size() * sizeof(uint32_t)));
    return (bool)f;
}

int main(int argc, char **argv) {
    if (mm_device_count() <= 0) return 77;
    if (argc != 3) {
        fprintf(stderr, "usage: %s DIR N_THREADS\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    const int n_threads = std::stoi(argv[2]);
    const auto builder = canonical_minimizers(21, 11);  // shared by every thread
    std::vector<int> status(n_threads, -1);
    std::vector<std::thread> threads;
    for (int t = 0; t < n_threads; ++t)
        threads.emplace_back([&, t] {
            try {
                const std::string in = dir + "/in_" + std::to_string(t) + "_", out = dir + "/out_" + std::to_string(t) + "_";
                unsigned long long n_packed = 0, n_nseq = 0;
                {
                    std::ifstream f(in + "len.txt");
                    f >> n_packed >> n_nseq;
                }
                const std::vector<uint8_t> packed = read_file(in + "packed.bin"), nseq = read_file(in + "nseq.bin"),
                                           amb = read_file(in + "amb.bin"), text = read_file(in + "text.bin");
                std::vector<uint32_t> pos, skip, tpos;
                builder.run(PackedSeq{packed.data(), 0, n_packed}, pos);
                builder.run_skip_ambiguous_windows(PackedNSeq{PackedSeq{nseq.data(), 0, n_nseq}, amb.data(), 0}, skip);
                builder.run(TextSeq{text.data(), text.size()}, tpos);
                const bool ok = write_file(out + "run.bin", pos) && write_file(out + "skip.bin", skip) &&
                                write_file(out + "text.bin", tpos);
                status[t] = ok ? 0 : 3;
            } catch (const Error &e) {
                fprintf(stderr, "thread %d: %s\n", t, e.what());
                status[t] = 4;
            }
        });
    for (auto &th : threads) th.join();
    for (int t = 0; t < n_threads; ++t)
        if (status[t] != 0) return status[t];
    printf("threads example ok: %d threads\n", n_threads);
    return 0;
}
