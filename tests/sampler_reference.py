"""Host reference of the library's randomness (numpy only): what every coefficient of every generated key and every fresh ciphertext must
be, given the 64-bit seed of a hooks build.  Written from the definitions in dacapo_amd/csrc/chacha.hpp and the sampler comments of
dacapo_amd/csrc/hevm_vm.hip, vectorised over whole polynomials; shared by tests/test_sampler_reference.py (CPU) and
tests/test_gpu_samplers.py (GPU), a helper module like gpu_helpers.py.

A draw is addressed, not streamed.  The word of coefficient k of a polynomial is word k % 8 of the ChaCha20 block
    counter = object << 20 | (k // 8)          nonce = epoch << 16 | attempt << 8 | domain
under one of two keys (`secret`: everything private; `pub`: the uniform halves that are published inside keys).  Who draws from which
(key, object, domain, epoch) is the address table, draws() below; docs/design/boundary_and_runtime.md ("Address scheme of the randomness") is the
other place that states it."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

# enum RngDomain
RNG_SK, RNG_PK_A, RNG_PK_E, RNG_KSK_A, RNG_KSK_E, RNG_ENC_U, RNG_ENC_E0, RNG_ENC_E1, RNG_ESK = 1, 2, 3, 4, 5, 6, 7, 8, 9

# key ids of the key-switching keys (an object is key_id * 64 + digit)
KEY_RELIN, KEY_SWK_DOWN, KEY_SWK_UP, KEY_GALOIS0 = 8, 9, 10, 16
PLAN_OBJECT0 = 1 << 32   # opcode-10 item k of a plan encrypts from object 2^32 + k; Encryptor::encrypt number n from object n

# field widths of the address
BLOCK_BITS, LIMB_SLOTS, DIGIT_SLOTS, ATTEMPTS, OBJECT_BITS = 20, 64, 64, 256, 44

_M64 = (1 << 64) - 1
_U32 = np.uint32


# ---- keys and block function -----------------------------------------------------------------------------------------------------------
def rng_keys_from_test_seed(seed: int) -> dict:
    """both ChaCha20 keys of a seeded (hooks-build) VM: sixteen 32-bit words from eight splitmix64 outputs, low half first; words 0..7
    are the `secret` key, words 8..15 the `pub` key"""
    words, z = [], seed & _M64
    for _ in range(8):
        z = (z + 0x9E3779B97F4A7C15) & _M64
        x = z
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
        x ^= x >> 31
        words += [x & 0xFFFFFFFF, x >> 32]
    return {"secret": np.array(words[:8], dtype=_U32), "pub": np.array(words[8:], dtype=_U32)}


def _rotl(x, n):
    return (x << _U32(n)) | (x >> _U32(32 - n))


def chacha20_blocks(key, counters, nonces) -> np.ndarray:
    """ChaCha20 block function (RFC 8439 section 2.3, with the original 64-bit counter / 64-bit nonce split of state words 12..15) for an
    array of counters (and one nonce, or one per counter): uint32[n][16]"""
    ctr = np.atleast_1d(np.asarray(counters, dtype=np.uint64))
    non = np.broadcast_to(np.asarray(nonces, dtype=np.uint64), ctr.shape)
    n = ctr.shape[0]
    lo32 = np.uint64(0xFFFFFFFF)
    init = [np.full(n, c, dtype=_U32) for c in (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)]
    init += [np.full(n, int(w), dtype=_U32) for w in np.asarray(key, dtype=_U32)]
    init += [(ctr & lo32).astype(_U32), (ctr >> np.uint64(32)).astype(_U32), (non & lo32).astype(_U32), (non >> np.uint64(32)).astype(_U32)]
    x = [v.copy() for v in init]

    def quarter(a, b, c, d):
        x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 16)
        x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 12)
        x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 8)
        x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 7)

    with np.errstate(over="ignore"):
        for _ in range(10):
            for col in range(4):
                quarter(col, 4 + col, 8 + col, 12 + col)
            for col in range(4):
                quarter(col, 4 + (col + 1) % 4, 8 + (col + 2) % 4, 12 + (col + 3) % 4)
        return np.stack([x[i] + init[i] for i in range(16)], axis=1)


def rng_counter(obj: int, block):
    return (np.uint64(obj << BLOCK_BITS) | (np.asarray(block, dtype=np.uint64) & np.uint64((1 << BLOCK_BITS) - 1)))


def rng_nonce(epoch: int, attempt: int, domain: int) -> int:
    return ((epoch << 16) & _M64) | ((attempt & 0xFF) << 8) | (domain & 0xFF)


def rng_words8(key, obj: int, block, epoch: int, attempt: int, domain: int) -> np.ndarray:
    """the eight 64-bit words of the block(s) covering coefficients 8 * block .. 8 * block + 7: uint64[..., 8] (little-endian word pairs)"""
    blk = np.asarray(block, dtype=np.uint64)
    o = chacha20_blocks(key, rng_counter(obj, blk.reshape(-1)), rng_nonce(epoch, attempt, domain)).astype(np.uint64)
    return (o[:, 0::2] | (o[:, 1::2] << np.uint64(32))).reshape(blk.shape + (8,))


def poly_words(key, obj: int, N: int, epoch: int, attempt: int, domain: int) -> np.ndarray:
    """the N words of one polynomial's coefficients, in coefficient order"""
    return rng_words8(key, obj, np.arange(N // 8), epoch, attempt, domain).reshape(N)


# ---- small samplers ----------------------------------------------------------------------------------------------------------------------
def ternary(w) -> np.ndarray:
    """uniform on {-1, 0, 1} from one word: its 2-bit groups from the bottom up, the first that is not 3, minus 1 (all 32 equal to 3: 0)"""
    w = np.asarray(w, dtype=np.uint64).copy()
    out = np.zeros(w.shape, dtype=np.int64)
    open_ = np.ones(w.shape, dtype=bool)
    for _ in range(32):
        g = (w & np.uint64(3)).astype(np.int64)
        take = open_ & (g != 3)
        out[take] = g[take] - 1
        open_ &= ~take
        if not open_.any():
            break
        w >>= np.uint64(2)
    return out


def cbd(w) -> np.ndarray:
    """centred binomial, 21 - 21 coin flips: popcount of bits 0..20 minus popcount of bits 21..41"""
    w = np.asarray(w, dtype=np.uint64)
    m = np.uint64((1 << 21) - 1)
    return np.bitwise_count(w & m).astype(np.int64) - np.bitwise_count((w >> np.uint64(21)) & m).astype(np.int64)


def small_poly(key, obj: int, N: int, domain: int, epoch: int = 0, kind: str = "cbd") -> np.ndarray:
    """one small signed polynomial (int64[N]); kind = "ternary" or "cbd" """
    w = poly_words(key, obj, N, epoch, 0, domain)
    return ternary(w) if kind == "ternary" else cbd(w)


def lift(v, primes) -> np.ndarray:
    """a signed polynomial as residues of each prime: uint64[len(primes)][N]"""
    v = np.asarray(v, dtype=np.int64)
    return np.stack([np.where(v < 0, v + np.int64(q), v).astype(np.uint64) for q in primes])


# ---- uniform sampler ---------------------------------------------------------------------------------------------------------------------
def uniform_limb(key, obj: int, q: int, N: int, domain: int):
    """uniform residues of one prime by rejection: a draw is the top b bits of the word, b the prime's own width; a draw >= q is replaced by
    the same word index of the block at attempt 1, 2, ... .  `obj` is the limb's own object.  Returns (uint64[N], retries uint8[N])."""
    sh = np.uint64(64 - int(q).bit_length())
    r = poly_words(key, obj, N, 0, 0, domain) >> sh
    retries = np.zeros(N, dtype=np.uint8)
    for attempt in range(1, ATTEMPTS):
        bad = np.nonzero(r >= np.uint64(q))[0]
        if bad.size == 0:
            break
        w = rng_words8(key, obj, bad // 8, 0, attempt, domain)
        r[bad] = w[np.arange(bad.size), bad % 8] >> sh
        retries[bad] += 1
    return r, retries


def uniform_poly(key, obj: int, primes, N: int, domain: int):
    """the uniform half of one key (digit): limb i draws from object obj * 64 + i.  Returns (uint64[K][N], retries uint8[K][N])."""
    both = [uniform_limb(key, obj * LIMB_SLOTS + i, q, N, domain) for i, q in enumerate(primes)]
    return np.stack([b[0] for b in both]), np.stack([b[1] for b in both])


# ---- sparse secret -----------------------------------------------------------------------------------------------------------------------
def sparse_secret(key, N: int, weight: int, domain: int) -> np.ndarray:
    """exactly `weight` coefficients +-1 (int64[N]): words of object 0, attempt 1, domain RNG_SK (option secret_hw) or RNG_ESK (option
    boot_secret_hw), taken in order; position (w >> 8) % N, sign +1 if w & 1 else -1; a word whose position is occupied is skipped"""
    coef = np.zeros(N, dtype=np.int64)
    placed, blk = 0, 0
    while placed < weight:
        for w in rng_words8(key, 0, np.arange(blk, blk + 64), 0, 1, domain).reshape(-1):
            idx = (int(w) >> 8) % N
            if coef[idx]:
                continue
            coef[idx] = 1 if int(w) & 1 else -1
            placed += 1
            if placed == weight:
                break
        blk += 64
    return coef


# ---- address table -----------------------------------------------------------------------------------------------------------------------
class Draw(NamedTuple):
    who: str        # what is drawn
    key: str        # "secret" or "pub"
    obj: int        # object
    domain: int
    epoch: int
    attempts: tuple  # (first, last + 1) attempt numbers the draw may use
    blocks: int     # consecutive block numbers, from 0


def galois_key_id(elt: int) -> int:
    return KEY_GALOIS0 + elt


def default_galois_elts(logN: int):
    """SEAL's GaloisTool::get_elts_all(): 2N - 1, then 3^(2^i) and 3^-(2^i) mod 2N for i < logN - 1"""
    m = 2 << logN
    pos, neg, out = 3, pow(3, -1, m), [m - 1]
    for _ in range(logN - 1):
        out += [pos] if pos == neg else [pos, neg]   # (the last pair is one element: 3^(N/4) is its own inverse)
        pos, neg = pos * pos % m, neg * neg % m
    return out


def kswitch_draws(who, key_id: int, digits: int, limbs: int, N: int):
    """digit j of key `key_id`: uniform half, limb i from object (key_id * 64 + j) * 64 + i of the public key, domain KSK_A; error from
    object key_id * 64 + j of the secret key, domain KSK_E"""
    nb = N // 8
    for j in range(digits):
        obj = key_id * DIGIT_SLOTS + j
        for i in range(limbs):
            yield Draw(f"{who} digit {j} a limb {i}", "pub", obj * LIMB_SLOTS + i, RNG_KSK_A, 0, (0, ATTEMPTS), nb)
        yield Draw(f"{who} digit {j} e", "secret", obj, RNG_KSK_E, 0, (0, 1), nb)


def draws(logN: int, limbs: int, digits: int, galois_elts=None, secret_hw: int = 0, boot=None, encryptions=(), plan_items=()):
    """Every draw the library makes for one VM.  limbs = primes of the chain, digits = digits per key-switching key (SEAL layout: limbs - 1).
    boot = (digits of swk_down, limbs of swk_down) with option boot_secret_hw (swk_up has the chain's shape).  encryptions: (n, epoch) of
    Encryptor::encrypt calls (n counts them over the VM's life, epoch = run() calls made before); plan_items: (k, epoch) of opcode-10 items
    of a plan."""
    N, nb = 1 << logN, (1 << logN) // 8
    if secret_hw:   # positions and signs come from as many words as it takes: bounded by the whole object here
        yield Draw("sk (sparse)", "secret", 0, RNG_SK, 0, (1, 2), nb)
    else:
        yield Draw("sk", "secret", 0, RNG_SK, 0, (0, 1), nb)
    for i in range(limbs):
        yield Draw(f"pk a limb {i}", "pub", i, RNG_PK_A, 0, (0, ATTEMPTS), nb)   # (object 0 of the uniform sampler: 0 * 64 + i)
    yield Draw("pk e", "secret", 0, RNG_PK_E, 0, (0, 1), nb)
    yield from kswitch_draws("relin", KEY_RELIN, digits, limbs, N)
    for elt in (default_galois_elts(logN) if galois_elts is None else galois_elts):
        yield from kswitch_draws(f"galois {elt}", galois_key_id(elt), digits, limbs, N)
    if boot:
        yield Draw("ephemeral sparse secret", "secret", 0, RNG_ESK, 0, (1, 2), nb)
        yield from kswitch_draws("swk_down", KEY_SWK_DOWN, boot[0], boot[1], N)
        yield from kswitch_draws("swk_up", KEY_SWK_UP, digits, limbs, N)
    for tag, base, items in (("encryption", 0, encryptions), ("opcode-10 item", PLAN_OBJECT0, plan_items)):
        for n, epoch in items:
            for name, dom in (("u", RNG_ENC_U), ("e0", RNG_ENC_E0), ("e1", RNG_ENC_E1)):
                yield Draw(f"{tag} {n} epoch {epoch} {name}", "secret", base + n, dom, epoch, (0, 1), nb)


# ---- whole objects, as the GPU tests compare them --------------------------------------------------------------------------------------
def kswitch_digit(keys, key_id: int, digit: int, primes, N: int):
    """digit `digit` of key `key_id`: (uniform half uint64[K][N], stored as drawn; error int64[N]; retries uint8[K][N])"""
    obj = key_id * DIGIT_SLOTS + digit
    a, retries = uniform_poly(keys["pub"], obj, primes, N, RNG_KSK_A)
    return a, small_poly(keys["secret"], obj, N, RNG_KSK_E), retries


def enc_sample(keys, obj: int, epoch: int, N: int):
    """(u, e0, e1) of one zero-encryption, int64[N] each: ternary u, centred-binomial errors"""
    s = keys["secret"]
    return (small_poly(s, obj, N, RNG_ENC_U, epoch, "ternary"), small_poly(s, obj, N, RNG_ENC_E0, epoch), small_poly(s, obj, N, RNG_ENC_E1, epoch))
