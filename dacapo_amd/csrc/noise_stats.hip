// Error statistics of polynomials on the device (noise_stats.hpp): D = m got - want is formed limb by limb in NTT form, brought to the
// coefficient domain by the library's batched inverse transform, and every coefficient is lifted from its residues to the centred
// integer it stands for -- from limb 0 alone at one limb, from limbs 0 and 1 by Garner otherwise; the further limbs only have to agree --
// and reduced: wave by cross-lane moves, workgroup through LDS, one record per workgroup, then one workgroup per polynomial adds the records
// in a fixed order.  No atomics: the same input gives the same bits on every run.
#include "noise_stats.hpp"

namespace dacapo {

namespace {

typedef unsigned __int128 d_u128;

__device__ __forceinline__ d_u128 make128(u64 hi, u64 lo) { return ((d_u128)hi << 64) | (d_u128)lo; }

// ---- (a) D = m got - want, canonical.  grid = (N / 512, ell, count) ------------------------------------------------------------------------
__global__ __launch_bounds__(kNoiseThreads) void noise_diff_kernel(u64 *__restrict__ D, const u64 *__restrict__ got, long got_stride,
                                                                    const u64 *__restrict__ want, long want_stride, int ell, size_t N,
                                                                    const DModulus *__restrict__ mods, int m_prime)
{
    const int i = blockIdx.y;
    const size_t b = blockIdx.z;
    const DModulus M = mods[i];
    const size_t k = ((size_t)blockIdx.x * kNoiseThreads + threadIdx.x) * 2;
    u64x2 g = *reinterpret_cast<const u64x2 *>(got + (long)b * got_stride + (long)i * (long)N + (long)k);
    if (m_prime >= 0) { // the multiplier's residue: another prime of the chain, possibly wider than this one
        const u64 m = canon(mods[m_prime].q, M);
#pragma unroll
        for (int t = 0; t < 2; t++) g[t] = mulmod(m, g[t], M);
    }
    if (want) {
        const u64x2 w = *reinterpret_cast<const u64x2 *>(want + (long)b * want_stride + (long)i * (long)N + (long)k);
#pragma unroll
        for (int t = 0; t < 2; t++) g[t] = submod(g[t], w[t], M.q);
    }
    *reinterpret_cast<u64x2 *>(D + (b * (size_t)ell + (size_t)i) * N + k) = g;
}

// ---- reductions ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void stats_add(NoiseStats &a, const NoiseStats &b)
{
    a.sum_sq += b.sum_sq;
    a.sum += b.sum;
    if (make128(b.max_hi, b.max_lo) > make128(a.max_hi, a.max_lo)) a.max_hi = b.max_hi, a.max_lo = b.max_lo;
    a.inconsistent += b.inconsistent;
}

// all 64 lanes end with the wave's total: lane L adds lane L ^ d for d = 32 .. 1, the same pairs in the same order on every run (a + b is
// b + a bit for bit, so the two lanes of a pair agree)
__device__ __forceinline__ void stats_wave_reduce(NoiseStats &a)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        NoiseStats o;
        o.sum_sq = __shfl_xor(a.sum_sq, d);
        o.sum = __shfl_xor(a.sum, d);
        o.max_lo = __shfl_xor((unsigned long long)a.max_lo, d);
        o.max_hi = __shfl_xor((unsigned long long)a.max_hi, d);
        o.inconsistent = __shfl_xor(a.inconsistent, d);
        stats_add(a, o);
    }
}

// ---- (c) lift and reduce.  grid = (N / 512, count): two adjacent coefficients per thread, every limb read as one 16-byte access ------------
// inv01 = (q0 mod q1)^-1 mod q1.  m: the divisor of the sums (1 or the multiplier prime), as a double.
__global__ __launch_bounds__(kNoiseThreads) void noise_lift_kernel(NoiseStats *__restrict__ part, const u64 *__restrict__ D, int ell, size_t N,
                                                                    const DModulus *__restrict__ mods, u64 inv01, double m)
{
    const size_t b = blockIdx.y;
    const size_t k = ((size_t)blockIdx.x * kNoiseThreads + threadIdx.x) * 2;
    const u64 *d = D + b * (size_t)ell * N + k;
    const u64 q0 = mods[0].q;
    const u64x2 r0 = *reinterpret_cast<const u64x2 *>(d);
    bool neg[2];
    d_u128 mag[2]; // |value|, value in (-M/2, M/2]: M is odd, so |value| <= (M - 1) / 2
    if (ell == 1) {
#pragma unroll
        for (int t = 0; t < 2; t++) {
            neg[t] = r0[t] > (q0 >> 1);
            mag[t] = neg[t] ? q0 - r0[t] : r0[t];
        }
    } else {
        const DModulus M1 = mods[1];
        const u64x2 r1 = *reinterpret_cast<const u64x2 *>(d + N);
        u64 mh, ml;
        mul_wide(q0, M1.q, mh, ml);
        const d_u128 M = make128(mh, ml), half = M >> 1;
#pragma unroll
        for (int t = 0; t < 2; t++) { // x = r0 + q0 ((r1 - r0) / q0 mod q1)  in [0, q0 q1)
            const u64 u = mulmod(inv01, submod(r1[t], canon(r0[t], M1), M1.q), M1);
            u64 ph, pl;
            mul_wide(q0, u, ph, pl);
            const d_u128 x = make128(ph, pl) + r0[t];
            neg[t] = x > half;
            mag[t] = neg[t] ? M - x : x;
        }
    }
    NoiseStats a{ 0.0, 0.0, 0, 0, 0 };
    for (int i = 2; i < ell; i++) { // the further limbs must hold the same integer (|value| < 2^119: reduce128_any's range)
        const DModulus Mi = mods[i];
        const u64x2 ri = *reinterpret_cast<const u64x2 *>(d + (size_t)i * N);
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const u64 r = reduce128_any((u64)(mag[t] >> 64), (u64)mag[t], Mi);
            a.inconsistent += (neg[t] ? negmod(r, Mi.q) : r) != ri[t];
        }
    }
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const double v = ((double)(u64)(mag[t] >> 64) * 0x1p64 + (double)(u64)mag[t]) / m;
        a.sum_sq += v * v;
        a.sum += neg[t] ? -v : v;
        if (mag[t] > make128(a.max_hi, a.max_lo)) a.max_hi = (u64)(mag[t] >> 64), a.max_lo = (u64)mag[t];
    }
    stats_wave_reduce(a);
    __shared__ NoiseStats waves[kNoiseThreads / 64];
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kNoiseThreads / 64; w++) stats_add(a, waves[w]);
        part[b * gridDim.x + blockIdx.x] = a;
    }
}

// ---- (d) finish.  grid = (count), one wave: lane L adds its run of consecutive records in index order, then the lanes are added ---------------
__global__ __launch_bounds__(64) void noise_finish_kernel(NoiseStats *__restrict__ out, const NoiseStats *__restrict__ part, int per_item)
{
    const int run = (per_item + 63) / 64, lo = (int)threadIdx.x * run, hi = min(lo + run, per_item);
    const NoiseStats *p = part + (size_t)blockIdx.x * (size_t)per_item;
    NoiseStats a{ 0.0, 0.0, 0, 0, 0 };
    for (int j = lo; j < hi; j++) stats_add(a, p[j]);
    stats_wave_reduce(a);
    if (threadIdx.x == 0) out[blockIdx.x] = a;
}

} // namespace

size_t noise_scratch_words(const Context &c, int ell, int count)
{
    const size_t per_item = c.N / kNoiseTile;
    return (size_t)count * (size_t)ell * c.N + ((size_t)count * per_item + (size_t)count) * (sizeof(NoiseStats) / sizeof(u64));
}

const NoiseStats *noise_error_stats(const Context &c, u64 *scratch, const u64 *got, long got_stride, const u64 *want, long want_stride, int ell,
                                    int count, int m_prime, hipStream_t s)
{
    static_assert(sizeof(NoiseStats) == 5 * sizeof(u64), "records are laid out in words");
    const size_t N = c.N;
    const unsigned tiles = (unsigned)(N / kNoiseTile);
    u64 *D = scratch;
    NoiseStats *part = reinterpret_cast<NoiseStats *>(scratch + (size_t)count * (size_t)ell * N), *total = part + (size_t)count * tiles;
    DC_LAUNCH(noise_diff_kernel, dim3(tiles, (unsigned)ell, (unsigned)count), dim3(kNoiseThreads), 0, s, D, got, got_stride, want, want_stride, ell, N,
              c.d_mods, m_prime);
    launch_ntt(c, true, D, (long)N, count * ell, nullptr, 0, ell, s);
    const u64 inv01 = ell >= 2 ? h_invmod(c.primes[0] % c.primes[1], c.primes[1]) : 0;
    const double m = m_prime >= 0 ? (double)c.primes[(size_t)m_prime] : 1.0;
    DC_LAUNCH(noise_lift_kernel, dim3(tiles, (unsigned)count), dim3(kNoiseThreads), 0, s, part, D, ell, N, c.d_mods, inv01, m);
    DC_LAUNCH(noise_finish_kernel, dim3((unsigned)count), dim3(64), 0, s, total, part, (int)tiles);
    return total;
}

} // namespace dacapo
