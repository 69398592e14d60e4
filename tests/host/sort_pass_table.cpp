// The pass table of a frame's sort run as gs_internal.h derives it, one line per pass:
//   <pass> <shift> <lo_in> <lo_out> <pk_in> <pk_out> <word16> <word_shift> <bytes read + written per element>
// usage: sort_pass_table <hi16 0|1> <num_gaussians> <num_sort_bits> <digit_bits> <fed 0|1> <record_timings>
// (tests/test_packed_words_cpu.py builds and runs it; host code only, nothing is launched)
#include <cstdio>
#include <cstdlib>

#include "gs_internal.h"

int main(int argc, char** argv) {
    if (argc != 7) return 2;
    const bool hi16 = std::atoi(argv[1]) != 0;
    const uint32_t n = (uint32_t)std::strtoul(argv[2], nullptr, 10);
    const uint32_t digit_bits = (uint32_t)std::atoi(argv[4]);
    gs::SortRun run;
    run.capacity = 1u << 20;
    run.num_sort_bits = (uint32_t)std::atoi(argv[3]);
    run.drop_depth_payload = true;
    run.hi16 = hi16;
    run.fed = std::atoi(argv[5]) != 0;
    run.packed = digit_bits == 4u && gs::frame_packs_payload(hi16, n, (uint32_t)std::atoi(argv[6]));     // what enqueue_frame sets for GS_SORT_RADIX4
    const uint32_t passes = gs::sort_pass_count(run, digit_bits);
    for (uint32_t k = 0; k < passes; ++k) {
        const gs::SortPass p = gs::sort_pass(run, digit_bits, k);
        std::printf("%u %u %d %d %d %d %d %u %u\n", k, p.shift, p.lo_in, p.lo_out, p.pk_in, p.pk_out, p.word16 ? 1 : 0,
                    p.word_shift, gs::sort_pass_bytes(p, hi16));
    }
    return 0;
}
