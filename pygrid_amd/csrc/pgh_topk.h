// Internal launcher interface of kernel K18 (pgh_topk.hip), beside pgh_kernels.h.  Not installed.
#pragma once
#include "pgh_kernels.h"

namespace pgh {

// Top-k sparsification of the averaged update behind a FINAL fold (the definition is in include/pgh_api.h):
// u = g + e, key = bits(u) & 0x7fffffff, tau = the k-th largest key, keep = key >= tau.  K18 is a three-digit
// MSB-first radix select over the 31-bit key -- digits of 11, 10 and 10 bits -- and one apply pass, five kinds
// of launch on one stream with no host round trip between them:
//   launch_topk_hist(digit 0)   d and e in, u out, the histogram of key >> 20
//   launch_topk_pick(digit 0)   the bin that holds rank k -> the state block; the histogram cleared
//   launch_topk_hist(1), pick(1), hist(2), pick(2)   the same walk over u, only keys under the prefix counted
//   launch_topk_apply           u, ckpt and tau in; out = ckpt - s (or d = -s ahead of K10) and the pending e' out
constexpr int TOPK_BINS = 2048;        // bins of the first digit (11 bits); the later digits use the first 1,024
constexpr int TOPK_WG_PARAMS = 1024;   // one 16-byte column per lane and sweep
constexpr int TOPK_MAX_WGS = 8192;     // grid-stride beyond
// The device-resident block: the histogram, then the selection's state.
struct TopkBlock {
    uint32_t hist[TOPK_BINS];
    uint32_t prefix;     // the digits chosen so far, right-aligned; after the third pick: tau
    uint32_t rank;       // the rank still to find among the keys under the prefix, 1-based from the top
    uint32_t n_eq;       // after the third pick: #{key == tau}
    uint32_t pad;
    uint64_t n_gt;       // #{key > the prefix's range}; after the third pick: #{key > tau}
};
struct TopkArgs {
    const float* d;      // hist(0): the delta plane, -g bit for bit, [p]
    const float* e;      // hist(0): the committed error memory [p], or null (no addition is made then)
    float* u;            // the work plane [p]: written by hist(0), read by every later launch
    const float* ckpt;   // apply: [p], or null when K10 follows
    float* out;          // apply: out = ckpt - s, or, with ckpt null, -s
    float* e2;           // apply: the pending error memory [p], or null
    TopkBlock* blk;
    int64_t p;
    uint32_t k;          // pick(0): the rank asked for, 1 <= k <= p
};
hipError_t launch_topk_hist(const TopkArgs& a, int digit, hipStream_t s);
hipError_t launch_topk_pick(const TopkArgs& a, int digit, hipStream_t s);
hipError_t launch_topk_apply(const TopkArgs& a, hipStream_t s);
hipError_t launch_topk_clear(TopkBlock* blk, hipStream_t s);  // the whole block to zero (a small kernel)

}  // namespace pgh
