// What the inner-product kernels of SEAL-layout key switching share -- f_ks_frows_mac_kernel (fused_ks.hip), f_ks_gmac_kernel and
// f_ks_gsum_kernel (hoist_ks.hip): the decode of a workgroup's row, the fold of an accumulator pair (the 16 products an Acc128 holds), and the
// host rule that picks their launch shape, whose grid order ks_row decodes.  One definition of each -- with one exception that is kept in step
// by hand: f_ks_frows_mac_kernel writes ks_row's and ks_fold's few lines out, because through the functions its compiled code changes (its
// assembly is held identical across refactors; profiles/ks_mac_regs.txt).  The hoisted kernels and all three launchers use what is here.
#pragma once
#include <type_traits>

#include "galois.hpp"
#include "ntt_tile.hpp"
#include "plan.hpp"
#include "tile_dispatch.hpp"

namespace dacapo {

// Workgroup (tile, y, b) of grid (tiles, l + 2 - MERGE, B) owns one ROWS-phase tile of output modulus slot m of item (hop, or group of a
// lazy sum) b: y < l is data prime y with both accumulators; above, the special prime (pm = the slot's prime in the key-level chain of Kp primes).
struct KsRow {
    int y, b, m, psel, pm;
};
template <bool MERGE, class BlockIdx> // (BlockIdx: the type of the builtin blockIdx, whose members are read where they are used)
__device__ __forceinline__ KsRow ks_row(const BlockIdx &bi, int ell, int Kp, int items_fast)
{
    // items_fast: grid = (tiles, B, rows) instead of (tiles, rows, B).  The workgroups (tile, row) of consecutive items are then 2^k tiles apart
    // in launch order -- the same XCD (workgroup w runs on XCD w mod 8), dispatched together -- and items that use the same key (the plan
    // sorts a rotation step's items by Galois element; a relinearisation step has one key) read each key tile out of that XCD's L2 after
    // the first of them fetched it.  SEAL's default key set has 28 elements, so a 64-item step of a convolution names each key several times:
    // with the rows slower than the items, two readers of a key tile were a whole item (~150 MB of traffic at 13 primes) apart.
    const int y = items_fast ? bi.z : bi.y, b = items_fast ? bi.y : bi.z, sp = Kp - 1;
    // psel < 0: both accumulators.  MERGE (grid.y = l + 1, throughput-bound launches): ONE workgroup row does the special prime for both
    // accumulators -- the l transforms of the lifted digits once instead of twice, then the two inverse ROWS phases one after the other
    // (its own instantiation: both accumulators live through the epilogue cost 16-20 VGPRs, a wave per SIMD)
    const int m = y < ell ? y : ell, psel = (MERGE && y == ell) ? -1 : y - ell;
    return KsRow{ y, b, m, psel, m == ell ? sp : m };
}

// a 128-bit accumulator holds 16 products of canonical residues (Acc128): fold the pair into canonical words, which then count as one more
// (tiny) term: 16 products + 2^60 < 2^124
template <int E>
__device__ __forceinline__ void ks_fold(Acc128 (&a0)[E], Acc128 (&a1)[E], const DModulus &M)
{
#pragma unroll
    for (int e = 0; e < E; e++) {
        const u64 f0 = a0[e].reduce(M), f1 = a1[e].reduce(M);
        a0[e].clear(), a1[e].clear();
        a0[e].lo = f0, a1[e].lo = f1;
    }
}

// (The hoisted digit step and the finish of a hoisted accumulator pair are NOT here: f_ks_gmac_kernel and f_ks_gsum_kernel each write them out.
// As functions they were built and compiled: the finish costs the merged LOGE = 2 forms of f_ks_gmac_kernel 1-3 VGPRs -- 127 -> 128 at N = 2^15,
// a wave per SIMD -- and f_ks_gsum_kernel<9, 2, true> nine, the digit step costs f_ks_gmac_kernel<K, 1, false> two; profiles/ks_mac_regs.txt.)

// ---- host: the launch shape of an inner-product kernel over `items` hops or groups at level l -----------------------------------------------
// tiny or small tiles (option tiny_tile_wgs); launches of at least ks_merge_special_min_wgs workgroups (more than the chip holds at once:
// throughput, not one workgroup's latency, is what counts) let one row of workgroups serve both special-prime accumulators, a huge value =
// never; the items-fast grid order (option ks_items_fast, ks_row) wherever the item count fits grid.y
// (the radix-8 geometry was measured for f_ks_frows_mac_kernel too: 8 coefficients x two 128-bit accumulators per thread cost more in
// occupancy than the saved LDS exchange returns -- config 3: 520 us against 455 us; profiles/r02_experiments.txt)
struct KsMacShape {
    int le, merge, items_fast;
    dim3 grid;
};
inline KsMacShape ks_mac_shape(const Context &c, int ell, int items)
{
    const int le = use_tiny_tiles(c.N, (long)(ell + 2) * items) ? 1 : 2;
    const unsigned tiles = (unsigned)(c.N >> (le == 1 ? TileGeo<1>::LOG : TileGeo<2>::LOG));
    const long wgs = (long)tiles * (ell + 2) * items;
    const int merge = wgs >= (long)option(OPT_KS_MERGE_SPECIAL_MIN_WGS) ? 1 : 0;
    const int items_fast = (items > 1 && items <= 65535 && option(OPT_KS_ITEMS_FAST)) ? 1 : 0;
    return { le, merge, items_fast, dim3(tiles, (unsigned)(items_fast ? items : ell + 2 - merge), (unsigned)(items_fast ? ell + 2 - merge : items)) };
}
// launch(K, LE, MERGE) with the three as std::integral_constant values: the caller names its kernel's instantiation with them
template <class Launch>
inline void ks_mac_dispatch(int k2, const KsMacShape &sh, Launch launch)
{
    auto with_k = [&](auto le, auto merge) { DC_K_SWITCH(k2, launch(std::integral_constant<int, KK>{}, le, merge)) };
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    if (sh.le == 1 && sh.merge)
        with_k(I1{}, std::true_type{});
    else if (sh.le == 1)
        with_k(I1{}, std::false_type{});
    else if (sh.merge)
        with_k(I2{}, std::true_type{});
    else
        with_k(I2{}, std::false_type{});
}

} // namespace dacapo
