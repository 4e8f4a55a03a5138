// Single-launch negacyclic NTT for the small rings, N = 2^12 .. 2^14: one workgroup owns one limb, reads it from HBM once, keeps ALL of it
// in LDS between its passes (32 / 64 / 128 KiB of the CU's 160 KiB) and writes it back once.  The two-launch tiles of ntt_tile.hpp cross
// HBM twice and, on these rings, are bound by their two dependent launches rather than by bytes.  The N = 2^15 kernel (ntt_full.hip) cannot
// work this way -- its limb is 256 KiB, so it lives in registers and moves through LDS in two rounds; here the limb fits, and the kernel is a
// plain sequence of in-place radix-16 passes over an LDS image.  Same butterflies (ntt_tile.hpp: ct_bfly / gs_bfly, forward folds by global
// stage), same word twiddle tables, every output canonical: results are bit-identical to the two-launch transform (tests/test_gpu_ntt_lds.py).
//
// Geometry.  T = N / 16 threads (1024 / 512 / 256), 16 coefficients per thread and pass in 32 VGPRs.  R0 = logN - 12 (2, 1, 0).
//
// Index algebra.  The LDS image is the limb in natural index order.  A pass holds one 4-bit field of the coefficient index in a thread's 16
// registers (register j <-> field value j) while the other logN - 4 bits are the thread: with LOB the field's position,
//         index = (tid >> LOB) << (LOB + 4)  |  j << LOB  |  tid & (2^LOB - 1)                     hi = tid >> LOB = the bits above the field
// Forward (Cooley-Tukey, natural in, bit-reversed out; stage s couples index bit logN - 1 - s and uses tw[2^s + (index >> (logN - s))]):
//     pass 0   stages 0 .. R0-1      field = bits logN-1 .. logN-4, of which only the top R0 are transformed (2^(4-R0) independent
//              (2^13, 2^14 only)     networks per thread); coefficients straight from HBM, index = j T + tid: 8 bytes per lane, lane-contiguous;
//                                    twiddles tw[2^s + (j >> ..)] depend on the register only -> scalar loads
//     pass A   stages R0 .. R0+3     LOB = 8, hi = tid >> 8 is wave-uniform -> 15 twiddles tw[2^s + (hi << t) + g] through scalar loads
//                                    (at 2^12 this is the first pass and reads HBM itself: index = j 256 + tid)
//     pass B   stages R0+4 .. R0+7   LOB = 4, hi = tid >> 4: four twiddle addresses per wave instruction (L1 broadcasts)
//     pass C   stages R0+8 .. R0+11  LOB = 0, hi = tid: a thread's 16 coefficients are adjacent; its 1 + 2 + 4 + 8 twiddles are contiguous per
//                                    thread and over the lanes (16-byte loads)
//     store    canonical values go back into the image; after a barrier the limb leaves with 16 bytes per lane, lane-contiguous (8 where the
//              limb is not 16-byte aligned)
// Inverse (Gentleman-Sande): the mirror image -- 16-byte loads into the image, passes C, B, A, 0 with the stages descending, N^-1 merged
// into global stage 0, and the last pass stores its registers straight to HBM (index = j T + tid).
// Every pass reads and writes the SAME image positions from the same thread, so a pass boundary is one barrier: nothing is read by another
// thread until the barrier, and nothing of the next pass is written before every read of this one has returned to its own thread.
// In-place operation on HBM is safe by construction: the first store follows at least one barrier after the last load.
//
// Bank conflicts.  Image position a is stored at a ^ ((a >> 4) & 31) (lds_sw): no padding, and for every access above the 32 lanes that
// share an LDS cycle (8-byte accesses) fall into 32 different 8-byte bank pairs:
//     LOB = 0 : a = tid 16 + j          low five bits (tid0, j) ^ tid[4:0]     -> (tid[3:0] ^ j, tid0 ^ tid4)  a bijection of tid[4:0]
//     LOB = 4 : a = hi 256 + j 16 + lo  low five bits (j0, lo) ^ (hi0, j)      -> (lo ^ j, j0 ^ hi0)           a bijection of (hi0, lo)
//     LOB >= 8: a = .. + lo             low five bits lo[4:0] ^ (c, lo[7:4])   -> a bijection of lo[4:0]       (lo[7:5], c constant per cycle)
// A 16-byte staging access covers positions 2P, 2P + 1: the swizzle moves them together and swaps them where bit 4 of 2P is set.
//
// Residency: 128 KiB + 1024 threads = one workgroup per CU at 2^14 (16 waves, 128 VGPRs each); 64 KiB x 2 at 2^13; 32 KiB x 4 or 5 at 2^12.
// The grid is persistent like ntt_full.hip's: as many workgroups as are resident (asked of the runtime), each walking over limbs prime by
// prime.  Compile-time resources: profiles/ntt_lds_regs.txt; what it buys and what bounds it: profiles/ntt_lds_ab.txt.
#include "kernels.hpp"
#include "ntt_tile.hpp"

namespace dacapo {

__device__ __forceinline__ int lds_sw(int a) { return a ^ ((a >> 4) & 31); }
// A fresh value as far as the optimiser can tell (no instruction): each section of a limb derives its addresses from the thread index where
// it uses them.  Otherwise the last section's sixteen 64-bit HBM addresses are formed at the top and spilled across the passes.
__device__ __forceinline__ void lds_launder(int &tid) { asm volatile("" : "+v"(tid)); }
// image position of register j of thread tid in a pass whose field sits at bit LOB
template <int LOB>
__device__ __forceinline__ int lds_idx(int tid, int j)
{
    return ((tid >> LOB) << (LOB + 4)) | (j << LOB) | (tid & ((1 << LOB) - 1));
}

// The pass's twiddles: w[2^t + g] = local stage t (global S0 + t), group g.  UNIFORM: hi is a scalar, the loads are scalar loads.
template <int S0, int NST, bool UNIFORM>
__device__ __forceinline__ void lds_twiddles(u64 (&w)[16], u32 hi, const u64 *__restrict__ tw)
{
#pragma unroll
    for (int t = 0; t < NST; t++) {
        const u64 *__restrict__ p = tw + ((size_t)1 << (S0 + t)) + ((size_t)hi << t);
        if constexpr (UNIFORM) {
#pragma unroll
            for (int g = 0; g < (1 << t); g++) w[(1 << t) + g] = p[g];
        } else if (t == 0)
            w[1] = p[0];
        else {
#pragma unroll
            for (int g = 0; g < (1 << t); g += 2) { // (p is 16-byte aligned: an even offset into a table that is)
                const u64x2 v = *reinterpret_cast<const u64x2 *>(p + g);
                w[(1 << t) + g] = v.x, w[(1 << t) + g + 1] = v.y;
            }
        }
    }
}

// NST stages of the radix-16 network on the register index, the first of them global stage S0: local stage t couples register bit 3 - t.
template <bool INV, int S0, int NST>
__device__ __forceinline__ void lds_stages(u64 (&x)[16], const u64 (&w)[16], const DModulus &M)
{
#pragma unroll
    for (int tt = 0; tt < NST; tt++) {
        const int t = INV ? NST - 1 - tt : tt, half = 8 >> t;
#pragma unroll
        for (int g = 0; g < (1 << t); g++) {
#pragma unroll
            for (int e = 0; e < half; e++) {
                const int j0 = (g << (4 - t)) | e, j1 = j0 | half;
                if constexpr (!INV)
                    ct_bfly(x[j0], x[j1], w[(1 << t) + g], M, fwd_stage_folds(S0 + t));
                else if (S0 + t == 0) { // the very last inverse stage carries N^-1
                    const u64 sv = x[j0] + x[j1], d = x[j0] + (M.q << 2) - x[j1];
                    x[j0] = mulmod_lazy(M.inv_n, sv, M.delta);
                    x[j1] = mulmod_lazy(M.inv_n_w, d, M.delta);
                } else
                    gs_bfly(x[j0], x[j1], w[(1 << t) + g], M);
                // four butterflies interleave, no more: eight (a whole stage) at once take the kernel past 128 VGPRs
                if (((g * half + e + 1) & 3) == 0) __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
}

// One full pass (four stages from global stage S0, field at bit LOB) over the image, in place.
// FROM_REGS: x[] already holds the pass's coefficients (the first forward pass at 2^12); TO_REGS: leave the result in x[] (the last inverse
// pass at 2^12); CANON: canonical values into the image (the last forward pass).
template <bool INV, int S0, int LOB, bool FROM_REGS, bool TO_REGS, bool CANON>
__device__ __forceinline__ void lds_pass(u64 (&x)[16], u64 *__restrict__ lds, int tid, const u64 *__restrict__ tw, const DModulus &M)
{
    constexpr bool UNIFORM = LOB >= 6; // hi = tid >> LOB is the same for the 64 lanes of a wave
    u64 w[16];
    lds_launder(tid);
    const u32 hi = UNIFORM ? (u32)__builtin_amdgcn_readfirstlane(tid >> LOB) : (u32)(tid >> LOB);
    lds_twiddles<S0, 4, UNIFORM>(w, hi, tw);
    if constexpr (!FROM_REGS) {
#pragma unroll
        for (int j = 0; j < 16; j++) x[j] = lds[lds_sw(lds_idx<LOB>(tid, j))];
    }
    lds_stages<INV, S0, 4>(x, w, M);
    if constexpr (!TO_REGS) {
#pragma unroll
        for (int j = 0; j < 16; j++) lds[lds_sw(lds_idx<LOB>(tid, j))] = CANON ? canon(x[j], M) : x[j];
        __syncthreads();
    }
}

// The limb between HBM and the image, lane-contiguous: 16 bytes per lane where the limb is 16-byte aligned (positions 2P, 2P + 1 are
// neighbours under lds_sw, swapped where bit 4 of 2P is set), 8 otherwise.
template <int T, bool TO_LDS>
__device__ __forceinline__ void lds_stage_limb(u64 *__restrict__ d, u64 *__restrict__ lds, int tid)
{
    if ((reinterpret_cast<size_t>(d) & 15) == 0) {
        u64x2 *__restrict__ d2 = reinterpret_cast<u64x2 *>(d);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int P = i * T + tid, sa = lds_sw(2 * P);
            u64x2 *__restrict__ l2 = reinterpret_cast<u64x2 *>(lds + (sa & ~1));
            if constexpr (TO_LDS) {
                const u64x2 v = d2[P];
                *l2 = (sa & 1) ? u64x2{ v.y, v.x } : v;
            } else {
                const u64x2 v = *l2;
                d2[P] = (sa & 1) ? u64x2{ v.y, v.x } : v;
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const int a = j * T + tid;
            if constexpr (TO_LDS)
                lds[lds_sw(a)] = d[a];
            else
                d[a] = lds[lds_sw(a)];
        }
    }
}

template <int LOGN, bool INV>
__device__ __forceinline__ void lds_limb(u64 *__restrict__ d, const u64 *__restrict__ tw, const DModulus &M, u64 *__restrict__ lds, int tid)
{
    constexpr int T = 1 << (LOGN - 4), R0 = LOGN - 12;
    u64 x[16];
    if constexpr (!INV) {
#pragma unroll
        for (int j = 0; j < 16; j++) x[j] = d[j * T + tid];
        if constexpr (R0 > 0) { // pass 0: the top R0 stages on the registers as loaded
            u64 w[16];
            lds_twiddles<0, R0, true>(w, 0, tw);
            lds_stages<false, 0, R0>(x, w, M);
#pragma unroll
            for (int j = 0; j < 16; j++) lds[lds_sw(j * T + tid)] = x[j];
            __syncthreads();
        }
        lds_pass<false, R0, 8, R0 == 0, false, false>(x, lds, tid, tw, M);
        lds_pass<false, R0 + 4, 4, false, false, false>(x, lds, tid, tw, M);
        lds_pass<false, R0 + 8, 0, false, false, true>(x, lds, tid, tw, M);
        lds_launder(tid);
        lds_stage_limb<T, false>(d, lds, tid);
    } else {
        lds_stage_limb<T, true>(d, lds, tid);
        __syncthreads();
        lds_pass<true, R0 + 8, 0, false, false, false>(x, lds, tid, tw, M);
        lds_pass<true, R0 + 4, 4, false, false, false>(x, lds, tid, tw, M);
        lds_pass<true, R0, 8, false, R0 == 0, false>(x, lds, tid, tw, M);
        lds_launder(tid);
        if constexpr (R0 > 0) {
            u64 w[16];
            lds_twiddles<0, R0, true>(w, 0, tw);
#pragma unroll
            for (int j = 0; j < 16; j++) x[j] = lds[lds_sw(j * T + tid)];
            lds_stages<true, 0, R0>(x, w, M);
        }
#pragma unroll
        for (int j = 0; j < 16; j++) d[j * T + tid] = canon(x[j], M);
    }
}

// grid = count (one limb per workgroup) or, above the number of resident workgroups, that number: each workgroup then walks over the limbs
// PRIME BY PRIME as ntt_full15_kernel does (limbs of residue 0 mod the period, then residue 1, ...: one or two twiddle tables in an XCD's L2
// at a time).  The thread index is laundered per iteration so that the passes' address arithmetic is not hoisted out of the loop into
// registers the butterflies need.  Four waves per SIMD (128 VGPRs) in every instantiation: at 2^14 that is the one workgroup its LDS
// allows, at 2^13 two workgroups and at 2^12 four, as many as their LDS images leave room for (five at 2^12, registers permitting).
template <int LOGN, bool INV>
__global__ __launch_bounds__(1 << (LOGN - 4)) __attribute__((amdgpu_waves_per_eu(4))) void ntt_lds_kernel(u64 *__restrict__ data, long limb_stride, const int *__restrict__ prime_idx,
                                                                   int prime_base, int prime_period, const DModulus *__restrict__ mods,
                                                                   const u64 *__restrict__ tw_all, int count)
{
    __shared__ __attribute__((aligned(16))) u64 lds[1 << LOGN];
    const int period = prime_period < count ? prime_period : count; // residues that occur
    const int big = count % period, ns = count / period, nb = ns + 1; // the first `big` residues have nb limbs, the others ns
    for (int pos = blockIdx.x; pos < count; pos += gridDim.x) {
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        int r, k;
        if (pos < big * nb)
            r = pos / nb, k = pos - r * nb;
        else {
            const int q = pos - big * nb;
            r = big + q / ns, k = q - (q / ns) * ns;
        }
        r = __builtin_amdgcn_readfirstlane(r), k = __builtin_amdgcn_readfirstlane(k);
        const int limb = k * period + r;
        const int p = prime_idx ? prime_idx[r] : prime_base + r;
        const DModulus M = mods[p];
        lds_limb<LOGN, INV>(data + (long)limb * limb_stride, tw_all + ((size_t)p << LOGN), M, lds, tid);
        __syncthreads(); // the next limb's first pass writes image positions that the slowest waves may still be reading
    }
}

bool ntt_lds_supported(const Context &c) { return c.logN >= 12 && c.logN <= 14; }

// Launches of at least this many limbs take this kernel instead of the two-launch tiles (options ntt_lds_min_limbs / ntt_lds_inv_min_limbs;
// 0 = never).  The defaults follow profiles/ntt_lds_ab.txt.
bool ntt_lds_pays(bool inverse, int count)
{
    const long m = (long)option(inverse ? OPT_NTT_LDS_INV_MIN_LIMBS : OPT_NTT_LDS_MIN_LIMBS);
    return m > 0 && count >= m;
}

// workgroups of this instantiation that the device holds at once: CUs x what LDS and registers allow per CU
template <int LOGN, bool INV>
static int lds_resident_wgs()
{
    static const int n = [] {
        int dev = 0, cus = 256, per = 1;
        if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, ntt_lds_kernel<LOGN, INV>, 1 << (LOGN - 4), 0) != hipSuccess || per < 1) per = 1;
        (void)hipGetLastError();
        return cus * per;
    }();
    return n;
}

template <int LOGN, bool INV>
static void launch_lds(const Context &c, u64 *data, long limb_stride, int count, const int *d_prime_idx, int prime_base, int prime_period,
                       hipStream_t s)
{
    const int res = lds_resident_wgs<LOGN, INV>();
    DC_LAUNCH((ntt_lds_kernel<LOGN, INV>), dim3((unsigned)(count > res ? res : count)), dim3(1u << (LOGN - 4)), 0, s, data, limb_stride,
              d_prime_idx, prime_base, prime_period, c.d_mods, INV ? c.d_itw : c.d_tw, count);
}

void launch_ntt_lds(const Context &c, bool inverse, u64 *data, long limb_stride, int count, const int *d_prime_idx, int prime_base,
                    int prime_period, hipStream_t s)
{
    if (count <= 0) return;
    if (prime_period <= 0) prime_period = 1 << 30;
#define DC_LDS(LN)                                                                                                    \
    case LN:                                                                                                          \
        if (inverse)                                                                                                  \
            launch_lds<LN, true>(c, data, limb_stride, count, d_prime_idx, prime_base, prime_period, s);             \
        else                                                                                                          \
            launch_lds<LN, false>(c, data, limb_stride, count, d_prime_idx, prime_base, prime_period, s);            \
        break;
    switch (c.logN) {
        DC_LDS(12)
        DC_LDS(13)
        DC_LDS(14)
    default: fprintf(stderr, "[dacapo_amd] launch_ntt_lds: N = 2^%d (the LDS-resident transform exists for 2^12 .. 2^14)\n", c.logN); abort();
    }
#undef DC_LDS
}

} // namespace dacapo
