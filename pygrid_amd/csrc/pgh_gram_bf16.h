// Internal launcher interface of kernel K20 (pgh_gram_bf16.hip), beside pgh_gram.h.  Not installed.
#pragma once
#include "pgh_api.h"
#include "pgh_gram.h"

namespace pgh {

// K20: the Gram matrix of the listed rows from split-bf16 products on the matrix cores (the definition is in
// include/pgh_api.h, "Split-bf16 Gram").  The arguments, the block pairs, the chunks, the partial blocks and the fold
// are K16's (GramArgs, pgh_gram.h); a.sums holds K7's sums of the listed rows by slab row, on the device before the
// launch.  A workgroup walks its chunk in steps of GRAM_BF16_KSTEP params and adds its f32 MFMA accumulators to
// the f64 ones every GRAM_BF16_RUN params (whole steps: a chunk is whole runs but for the shard's tail).
constexpr int GRAM_BF16_KSTEP = 32;
constexpr int GRAM_BF16_RUN = PGH_GRAM_BF16_RUN;
static_assert(GRAM_BF16_RUN % GRAM_BF16_KSTEP == 0 && SUMSQ_TILE % GRAM_BF16_RUN == 0, "K20: a run is whole steps, a tile whole runs");
hipError_t launch_row_gram_bf16(const GramArgs& a, hipStream_t s);

}  // namespace pgh
