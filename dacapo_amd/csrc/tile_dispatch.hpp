// Launch dispatch shared by the fused phase kernels (fused_ks.hip, hybrid_fused.hip): the phase size K is a template parameter of the tile
// routine (ntt_tile.hpp), the tile geometry is chosen per launch from its workgroup count.
#pragma once
#include "ntt_tile.hpp"

#define DC_K_SWITCH(Kval, ...)                                                                            \
    switch (Kval) {                                                                                       \
    case 6: { constexpr int KK = 6; __VA_ARGS__; } break;                                                        \
    case 7: { constexpr int KK = 7; __VA_ARGS__; } break;                                                        \
    case 8: { constexpr int KK = 8; __VA_ARGS__; } break;                                                        \
    case 9: { constexpr int KK = 9; __VA_ARGS__; } break;                                                        \
    default: fprintf(stderr, "[dacapo_amd] unsupported NTT phase size 2^%d\n", Kval); abort();             \
    }
// CALL sees KK (phase size) and LE (log2 coefficients per thread); grid.x = tiles of that geometry
#define DC_GEO_SWITCH(Kval, limbs, ...)                                                                   \
    if (use_tiny_tiles(c.N, (limbs))) {                                                                   \
        constexpr int LE = 1;                                                                             \
        const dim3 grid((unsigned)(c.N >> TileGeo<LE>::LOG), (unsigned)(limbs));                          \
        DC_K_SWITCH(Kval, __VA_ARGS__)                                                                         \
    } else if (use_small_tiles(c.N, (limbs))) {                                                           \
        constexpr int LE = 2;                                                                             \
        const dim3 grid((unsigned)(c.N >> TileGeo<LE>::LOG), (unsigned)(limbs));                          \
        DC_K_SWITCH(Kval, __VA_ARGS__)                                                                         \
    } else {                                                                                              \
        constexpr int LE = 3;                                                                             \
        const dim3 grid((unsigned)(c.N >> TileGeo<LE>::LOG), (unsigned)(limbs));                          \
        DC_K_SWITCH(Kval, __VA_ARGS__)                                                                         \
    }

namespace dacapo {

// The same choice as a function, for launches whose grid is not (tiles, limbs): log2 coefficients per thread of the geometry DC_GEO_SWITCH
// takes for `limbs`, its tile size, and launch(K, LE) with both as std::integral_constant values (ks_mac.hpp ks_mac_dispatch has the form)
inline int tile_geo_le(size_t N, long limbs) { return use_tiny_tiles(N, limbs) ? 1 : use_small_tiles(N, limbs) ? 2 : 3; }
inline int tile_geo_log(int le) { return le == 1 ? TileGeo<1>::LOG : le == 2 ? TileGeo<2>::LOG : TileGeo<3>::LOG; }
template <class Launch>
inline void tile_dispatch(int k, int le, Launch launch)
{
    auto with_k = [&](auto le_c) { DC_K_SWITCH(k, launch(std::integral_constant<int, KK>{}, le_c)) };
    if (le == 1)
        with_k(std::integral_constant<int, 1>{});
    else if (le == 2)
        with_k(std::integral_constant<int, 2>{});
    else
        with_k(std::integral_constant<int, 3>{});
}

} // namespace dacapo
