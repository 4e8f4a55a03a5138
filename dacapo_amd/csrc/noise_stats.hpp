// Error statistics of polynomials (dc_poly_error_stats, include/dacapo_ckks.h): how far `got` is from `want`, as exact integers lifted from
// the residues, reduced on the device (noise_stats.hip).  The sequence is four launches (+ the inverse transform's own one or two) whatever
// the number of polynomials: difference, the project's batched inverse transform, lift-and-reduce, finish.
#pragma once
#include "kernels.hpp"

namespace dacapo {

// One record of statistics: a workgroup's partial, and an item's total -- the layout of dc_error_stats.
struct NoiseStats {
    double sum_sq, sum;    // of D_j / m
    u64 max_lo, max_hi;    // max |D_j|, 128 bits
    long long inconsistent; // coefficients whose limbs >= 2 contradict the value lifted from limbs 0 and 1
};

constexpr int kNoiseThreads = 256;
constexpr int kNoiseTile = 2 * kNoiseThreads; // coefficients per workgroup of the lift-and-reduce kernel

// words of scratch `count` polynomials of `ell` limbs need: the difference [count][ell][N], the partials [count][N / kNoiseTile], the
// totals [count], the multiplier's residues [ell]
size_t noise_scratch_words(const Context &c, int ell, int count);

// D = m got - want (want may be null = 0; m_prime < 0: m = 1, else m = q_{m_prime}) over limbs 0 .. ell-1 of `count` polynomials, NTT form
// in, and the statistics of the centred integer D / m per polynomial into scratch; returns the device array of `count` totals (valid
// once the stream has run).  scratch: noise_scratch_words() words.
const NoiseStats *noise_error_stats(const Context &c, u64 *scratch, const u64 *got, long got_stride, const u64 *want, long want_stride, int ell,
                                    int count, int m_prime, hipStream_t s);

} // namespace dacapo
