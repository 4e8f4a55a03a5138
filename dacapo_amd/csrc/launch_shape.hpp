// Which launch sequence a SEAL-layout key switch takes: the ONE statement of the rule.  The launchers (batch_ops.hip, hoist_ks.hip), the plan
// (plan_exec.hip) and the C entry points (c_api.hip) ask here, and no other file reads options ks_big_tiles, ks_fuse_mac and ks_fuse_mac_tiles.
#pragma once
#include <cstddef>

#include "options.hpp"

namespace dacapo {

struct KsShape {
    long tiles;     // the batch's work in 1024-coefficient tiles of lifted digits
    bool big;       // large-batch sequence: inverse COLS phases once per limb, then base change + forward (25-35 % less work); else one launch (latency)
    bool fused_mac; // second NTT phase, inner products and the special prime's first inverse phase in one launch (by default always)
    bool hybrid;    // grouped-digit key switching: neither form below exists
    int ell;
    // a rescale folds into the multiply's key switch (b_mul_relin_rescale): the folded form exists for the latency-shaped sequence only
    bool folds_rescale() const { return !hybrid && ell >= 2 && fused_mac && !big; }
    // ... and into the grouped-digit multiply's mod-down (hybrid_fused.hip hybf_mul_relin_rescale_tail): the fused sequence, any batch size
    bool hyb_folds_rescale() const { return hybrid && ell >= 2 && option(OPT_HYB_FUSE) != 0; }
    // an item may carry an addend (KsItem::add): a start value of the fused middle's accumulators and of nothing else
    bool carries_addend() const { return !hybrid && fused_mac; }
};
inline KsShape ks_shape(size_t N, bool hybrid, int B, int ell)
{
    const long tiles = (long)(N >> 10) * B * ell * ell;
    return KsShape{ tiles, tiles >= (long)option(OPT_KS_BIG_TILES), option(OPT_KS_FUSE_MAC) != 0 && tiles < (long)option(OPT_KS_FUSE_MAC_TILES),
                    hybrid, ell };
}
// may chained steps hand off?  With ks_fuse_mac_tiles set, a linked step could fall on the un-fused middle, whose last kernel has no continuation form
inline bool chain_fusion_supported() { return option(OPT_KS_FUSE_MAC) != 0 && option(OPT_KS_FUSE_MAC_TILES) == (1LL << 40); }

} // namespace dacapo
