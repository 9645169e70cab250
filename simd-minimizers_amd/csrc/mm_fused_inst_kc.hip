// Fixed-k instances of the fused kernel (a file of their own so that the build parallelises): minimizers with k a
// compile-time constant, which lets the walk keep ONE sequence load stream (kc_rule, mm_fused_impl.h).
// canonical k=21 w=11 (the headline, BASELINE config 3).  Forward k=21 w=11 (config 2) is built only with -DMM_KC_FORWARD:
// it measured no faster than the run-time-k kernel (profiles/r07_one_stream_ab.txt).  k=31 w=51 (config 4) has no such
// form - its load groups are no whole number of bytes - and stays with the run-time-k kernel.
#include "mm_fused_impl.h"
#include "mm_fused_inst.h"

namespace mm {

#ifndef MM_NO_KC
static_assert(kc_rule(11, 21), "k=21 w=11 walks with one load stream");
static_assert(!kc_rule(51, 31), "k=31 w=51: listed here once the rule admits it");
#ifndef MM_EAGER_COUNT
static_assert(kc_count_rule(11, 21), "k=21 w=11 counts a tied window's strand from the hash-in buffers");
#endif
static_assert(!kc_count_rule(51, 31) && !kc_count_rule(11, 0), "no count plan without the one load stream");
#endif

const FusedKcInstance *fused_kc_instances(int *count) {
#ifndef MM_NO_KC
    static const FusedKcInstance kInst[] = {
        MM_KC_INST(11, 21, true, true),
#ifdef MM_KC_FORWARD  // (measured equal to the run-time-k kernel on 3.1 Gbp, 1.028 ms either way: not in the default dispatch)
        MM_KC_INST(11, 21, false, false),
#endif
    };
    *count = (int)(sizeof(kInst) / sizeof(kInst[0]));
    return kInst;
#else
    *count = 0;
    return nullptr;
#endif
}

}  // namespace mm
