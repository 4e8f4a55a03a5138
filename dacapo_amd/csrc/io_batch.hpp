// Batched encrypt / decrypt of all ciphertext streams (hevm_encrypt_batch / hevm_decrypt_batch, include/hevm_abi.h): the kernels the
// single-stream paths of hevm_vm.hip and encoder.hip have one item at a time, with the item in grid.y / grid.z (io_batch.hip).  The
// sequences themselves are HEVM::encrypt_batch / HEVM::decrypt_batch (hevm_vm.hip, "encode / encrypt / decrypt").
#pragma once
#include "crt_device.hpp"
#include "encoder.hpp"
#include "kernels.hpp"

namespace dacapo {

// Encryptor::encrypt's last step for B items: c0 of dst[b] += pt[b] (pt [B][ell][N], NTT form).  set: the zero-encryption test hook's
// (plaintext, 0) instead -- c0 = pt[b], c1 = 0.  One launch.
void io_add_plain(const Context &c, const CtView *d_dst, const u64 *pt, int B, int ell, bool set, hipStream_t s);
// Decryptor::decrypt's first step for B items and nothing after it: out[b] = c0 + c1 s of register slice src[b] over limbs 0 .. ell-1, NTT
// form (the polynomial that decrypt goes on to transform and decode; hevm_phase_batch).  One launch.
void io_phase(const Context &c, u64 *out, long out_stride, const CtView *d_src, const u64 *sk, int B, int ell, hipStream_t s);
// dec_crt_kernel for B items: coef [B][ell][N] (coefficient domain, canonical) -> v [B][N] complex, real parts = centred coefficient / scale.
// One launch.
void io_dec_crt(const Context &c, double2 *v, const u64 *coef, int B, int ell, CrtDev crt, double inv_scale, hipStream_t s);
// dec_fft for B items: v [B][N] -> out + b * out_stride, N/2 slot values each (out: device memory).  The butterflies and their order are
// dec_fft's, so every double is.  logN + 1 launches whatever B is.
void io_dec_fft(const Context &c, const EncTables &tb, double2 *v, double *out, long out_stride, int B, hipStream_t s);

} // namespace dacapo
