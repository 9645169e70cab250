// Reads-mode instances of the fused kernel for closed syncmers, open syncmers and minimizers + super-k-mer indices:
// canonical w = 15 and forward w = 17 (six kernels; see FusedReadsFlavourInstance in mm_fused_inst.h).
#include "mm_fused_impl.h"
#include "mm_fused_inst.h"

namespace mm {

const FusedReadsFlavourInstance *fused_reads_flavours_j(int *count) {
    static const FusedReadsFlavourInstance kInst[] = {
        MM_READS_FLAVOURS(15, true, true),
        MM_READS_FLAVOURS(17, false, false),
    };
    *count = (int)(sizeof(kInst) / sizeof(kInst[0]));
    return kInst;
}

}  // namespace mm
