// Batched encrypt / decrypt of all ciphertext streams: the item-indexed forms of the kernels that the single-stream paths run once per
// call (io_batch.hpp).  Nothing here changes an operation or its order -- an item's limbs and doubles are what `encrypt` / `decrypt` give.
#include "io_batch.hpp"

namespace dacapo {

constexpr int kIoThreads = 256;

// ---- encrypt: + plaintext on c0 ---------------------------------------------------------------------------------------------------------
// grid = (N/512, ell, B).  dst[b] is a register slice [2][capacity][N]; pt [B][ell][N].
__global__ __launch_bounds__(kIoThreads) void io_add_plain_kernel(const CtView *__restrict__ dst, const u64 *__restrict__ pt, int ell, size_t N,
                                                                   const DModulus *__restrict__ mods, int set)
{
    const int i = blockIdx.y, b = blockIdx.z;
    const u64 q = mods[i].q;
    const CtView d = dst[b];
    const size_t k = ((size_t)blockIdx.x * kIoThreads + threadIdx.x) * 2;
    const u64x2 m = *reinterpret_cast<const u64x2 *>(pt + ((size_t)b * ell + i) * N + k);
    u64x2 *c0 = reinterpret_cast<u64x2 *>(d.limb(0, i, N) + k);
    if (set) {
        *c0 = m;
        *reinterpret_cast<u64x2 *>(d.limb(1, i, N) + k) = u64x2{ 0, 0 };
    } else {
        const u64x2 z = *c0;
        *c0 = u64x2{ addmod(z.x, m.x, q), addmod(z.y, m.y, q) };
    }
}

void io_add_plain(const Context &c, const CtView *d_dst, const u64 *pt, int B, int ell, bool set, hipStream_t s)
{
    DC_LAUNCH(io_add_plain_kernel, dim3((unsigned)(c.N / (2 * kIoThreads)), (unsigned)ell, (unsigned)B), dim3(kIoThreads), 0, s, d_dst, pt, ell,
              c.N, c.d_mods, set ? 1 : 0);
}

// ---- phase: c0 + c1 s of B register slices (decrypt_kernel of hevm_vm.hip with the item in grid.z) ---------------------------------------
// grid = (N/512, ell, B).  src[b] is a register slice; out [B] polynomials [ell][N], out_stride words apart.
__global__ __launch_bounds__(kIoThreads) void io_phase_kernel(u64 *__restrict__ out, long out_stride, const CtView *__restrict__ src,
                                                               const u64 *__restrict__ sk, size_t N, const DModulus *__restrict__ mods)
{
    const int i = blockIdx.y, b = blockIdx.z;
    const DModulus M = mods[i];
    const CtView ct = src[b];
    const size_t k = ((size_t)blockIdx.x * kIoThreads + threadIdx.x) * 2;
    const u64x2 c0 = *reinterpret_cast<const u64x2 *>(ct.limb(0, i, N) + k), c1 = *reinterpret_cast<const u64x2 *>(ct.limb(1, i, N) + k),
                s = *reinterpret_cast<const u64x2 *>(sk + (size_t)i * N + k);
    u64x2 r;
#pragma unroll
    for (int t = 0; t < 2; t++) r[t] = addmod(c0[t], mulmod(c1[t], s[t], M), M.q);
    *reinterpret_cast<u64x2 *>(out + (long)b * out_stride + (long)i * (long)N + (long)k) = r;
}

void io_phase(const Context &c, u64 *out, long out_stride, const CtView *d_src, const u64 *sk, int B, int ell, hipStream_t s)
{
    DC_LAUNCH(io_phase_kernel, dim3((unsigned)(c.N / (2 * kIoThreads)), (unsigned)ell, (unsigned)B), dim3(kIoThreads), 0, s, out, out_stride, d_src,
              sk, c.N, c.d_mods);
}

// ---- decrypt: compose, centre, divide by the scale (dec_crt_kernel of hevm_vm.hip with the item in grid.y) --------------------------------
// grid = (N/256, B).  (Compiled like that kernel: the composition's sum of products is contracted the same way.)
__global__ __launch_bounds__(kIoThreads) void io_dec_crt_kernel(double2 *__restrict__ v, const u64 *__restrict__ coef, int ell, size_t N,
                                                                 const DModulus *__restrict__ mods, const CrtDev c, double inv_scale)
{
    const size_t n = (size_t)blockIdx.x * kIoThreads + threadIdx.x;
    const size_t b = blockIdx.y;
    v[b * N + n] = make_double2(crt_centered(coef + b * (size_t)ell * N, n, ell, N, mods, c) * inv_scale, 0.0);
}

void io_dec_crt(const Context &c, double2 *v, const u64 *coef, int B, int ell, CrtDev crt, double inv_scale, hipStream_t s)
{
    DC_LAUNCH(io_dec_crt_kernel, dim3((unsigned)(c.N / kIoThreads), (unsigned)B), dim3(kIoThreads), 0, s, v, coef, ell, c.N, c.d_mods, crt,
              inv_scale);
}

// ---- decrypt: forward special FFT and slot gather (dec_stage_kernel / dec_gather_kernel of encoder.hip with the item in grid.y) ---------
// IEEE double with contraction disabled from here on, as in encoder.hip: the butterflies are HostEncoder::decode's operation for operation.
#pragma clang fp contract(off)

__device__ __forceinline__ double2 io_cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// one Cooley-Tukey stage of transform_to_rev: group i of m, butterfly j of gap.  grid = (N/2/256, B)
__global__ __launch_bounds__(kIoThreads) void io_dec_stage_kernel(double2 *__restrict__ v, const double2 *__restrict__ roots, size_t N,
                                                                   unsigned log_gap)
{
    const size_t t = (size_t)blockIdx.x * kIoThreads + threadIdx.x;
    const size_t gap = (size_t)1 << log_gap, i = t >> log_gap, j = t & (gap - 1), m = (N >> 1) >> log_gap;
    double2 *x = v + (size_t)blockIdx.y * N + 2 * i * gap + j, *y = x + gap;
    const double2 a = *x, b = io_cmul(*y, roots[m + i]);
    *x = make_double2(a.x + b.x, a.y + b.y);
    *y = make_double2(a.x - b.x, a.y - b.y);
}

// out[b * out_stride + i] = Re v[b][slot_map[i]] for the N/2 slots.  grid = (N/2/256, B)
__global__ __launch_bounds__(kIoThreads) void io_dec_gather_kernel(double *__restrict__ out, long out_stride, const double2 *__restrict__ v,
                                                                    const u32 *__restrict__ slot_map, size_t N)
{
    const size_t i = (size_t)blockIdx.x * kIoThreads + threadIdx.x;
    out[(long)blockIdx.y * out_stride + (long)i] = v[(size_t)blockIdx.y * N + slot_map[i]].x;
}

void io_dec_fft(const Context &c, const EncTables &tb, double2 *v, double *out, long out_stride, int B, hipStream_t s)
{
    const size_t N = c.N;
    const dim3 grid((unsigned)(N / 2 / kIoThreads), (unsigned)B);
    for (int lg = c.logN - 1; lg >= 0; lg--) // m = 1, 2, ..., N/2  <=>  gap = N/2, ..., 1
        DC_LAUNCH(io_dec_stage_kernel, grid, dim3(kIoThreads), 0, s, v, tb.roots, N, (unsigned)lg);
    DC_LAUNCH(io_dec_gather_kernel, grid, dim3(kIoThreads), 0, s, out, out_stride, v, tb.slot_map, N);
}

} // namespace dacapo
