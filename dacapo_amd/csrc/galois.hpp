// The NTT-domain Galois permutation, once: the index map and the 16-byte gather every kernel that reads an operand through a rotation uses.
#pragma once
#include "modarith.hpp"

namespace dacapo {

// GaloisTool::apply_galois_ntt: out[k] = in[bitrev(((elt * (2*bitrev(k)+1)) >> 1) mod N)].  An aligned block of
// 2^b consecutive k reads an aligned block of 2^b consecutive inputs (elt is odd), so the gather stays
// coalesced at 64-lane granularity; no permutation table is needed (v_bfrev_b32 does the bit reversals).
__device__ __forceinline__ u32 galois_idx(u32 k, u32 elt, int logN)
{
    const u32 r = (__brev(k) >> (32 - logN)) * 2u + 1u;
    const u32 idx = ((elt * r) >> 1) & ((1u << logN) - 1u);
    return __brev(idx) >> (32 - logN);
}

// E consecutive coefficients k0 .. k0 + E - 1 (k0 a multiple of E >= 2) of galois(p): the index map sends an aligned pair of outputs to an
// aligned pair of inputs, possibly swapped (brev(k + 1) = brev(k) + N/2, elt odd: the source index moves by N/2 before its own bit
// reversal, i.e. its lowest bit flips), so a pair is ONE 16-byte load.  gi[h] is the source index of output k0 + 2h: a kernel that reads
// several limbs through one permutation (the digits of a hoisted hop) computes the pair indices once and gathers with them every time.
template <int E>
__device__ __forceinline__ void galois_pair_idx(u32 (&gi)[E / 2], u32 k0, u32 elt, int logN)
{
    static_assert(E >= 2 && E % 2 == 0, "pairs");
#pragma unroll
    for (int h = 0; h < E / 2; h++) gi[h] = galois_idx(k0 + 2u * (u32)h, elt, logN);
}
template <int E>
__device__ __forceinline__ void galois_gather(u64 (&x)[E], const u64 *__restrict__ p, const u32 (&gi)[E / 2])
{
#pragma unroll
    for (int h = 0; h < E / 2; h++) {
        const u64x2 v = *reinterpret_cast<const u64x2 *>(p + (gi[h] & ~1u));
        x[2 * h] = (gi[h] & 1u) ? v.y : v.x, x[2 * h + 1] = (gi[h] & 1u) ? v.x : v.y;
    }
}
// (the same gather with the indices computed on the way; written out rather than through the form above, which changes the code of
// f_ks_frows_mac_kernel and f_irows_rot_kernel)
template <int E>
__device__ __forceinline__ void galois_gather(u64 (&x)[E], const u64 *__restrict__ p, u32 k0, u32 elt, int logN)
{
    static_assert(E >= 2 && E % 2 == 0, "pairs");
#pragma unroll
    for (int e = 0; e < E; e += 2) {
        const u32 gi = galois_idx(k0 + (u32)e, elt, logN);
        const u64x2 v = *reinterpret_cast<const u64x2 *>(p + (gi & ~1u));
        x[e] = (gi & 1u) ? v.y : v.x, x[e + 1] = (gi & 1u) ? v.x : v.y;
    }
}

} // namespace dacapo
