"""CPU: the host reference of the library's randomness (tests/sampler_reference.py), which tests/test_gpu_samplers.py holds the device
samplers, key generation and encryption to, coefficient for coefficient.
  * its ChaCha20 block function is the library's own host one (hevm_chacha20_block) on the RFC 8439 vector and on random inputs;
  * the definitions are the distributions they claim to be: ternary uniform on {-1, 0, 1}, centred binomial Binomial(42, 1/2) - 21, uniform
    residues uniform on [0, q) -- chi-square tests on 2^20 draws of one fixed seed (a fixed input: nothing is flaky), each statistic
    bounded by the 1 - 10^-6 quantile of the chi-square law at its degrees of freedom;
  * the address table: no two draws of a VM share a ChaCha20 block under the same key and nonce, and every quantity fits its field (the
    limits this implies, at most 64 limbs and 64 digits per key, are what Context refuses to exceed: tests/test_gpu_samplers.py)."""
import ctypes as C
import math
from collections import defaultdict

import numpy as np
import pytest

import sampler_reference as sr
from dacapo_amd import LIB_PATH

SEED = 0x4845564D
DRAWS = 1 << 20
Q60, Q46 = 0xffffffffffc0001, 0x3ffff001e001   # the reference chain's top prime; the smallest 46-bit prime = 1 mod 2^13 with 2^46 - q < 2^28


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(str(LIB_PATH))
    L.hevm_chacha20_block.argtypes = [C.POINTER(C.c_uint32), C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32)]   # as in tests/test_seal_format.py
    return L


def lib_block(lib, key_words, counter, nonce):
    key, out = (C.c_uint32 * 8)(*[int(w) for w in key_words]), (C.c_uint32 * 16)()
    lib.hevm_chacha20_block(key, counter, nonce, out)
    return list(out)


# ---- block function, keys ---------------------------------------------------------------------------------------------------------------
def test_block_function_equals_the_librarys_on_the_rfc_vector_and_random_inputs(lib):
    import struct

    key = list(struct.unpack("<8I", bytes(range(32))))           # RFC 8439 section 2.3.2: counter 1, nonce 00:00:00:09 00:00:00:4a 00:00:00:00
    ctr, nonce = 1 | (0x09000000 << 32), 0x4A000000
    got = sr.chacha20_blocks(key, [ctr], nonce)[0]
    assert [int(x) for x in got[:4]] == [0xE4E7F110, 0x15593BD1, 0x1FDD0F50, 0xC47120A3]
    assert [int(x) for x in got] == lib_block(lib, key, ctr, nonce)
    rng = np.random.default_rng(3)
    for _ in range(8):                                            # several counters and per-counter nonces in one vectorised call
        key = [int(x) for x in rng.integers(0, 1 << 32, size=8)]
        ctrs = rng.integers(0, 1 << 63, size=6, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        nonces = rng.integers(0, 1 << 63, size=6, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=6, dtype=np.uint64)
        got = sr.chacha20_blocks(key, ctrs, nonces)
        for b in range(6):
            assert [int(x) for x in got[b]] == lib_block(lib, key, int(ctrs[b]), int(nonces[b]))


def test_words8_addressing_is_counter_and_nonce_of_the_definition(lib):
    keys = sr.rng_keys_from_test_seed(SEED)
    obj, block, epoch, attempt, domain = (1 << 32) + 5, 0x812AB, 3, 2, sr.RNG_ENC_E1
    w = sr.rng_words8(keys["secret"], obj, block, epoch, attempt, domain)
    o = lib_block(lib, keys["secret"], (obj << 20) | block, (epoch << 16) | (attempt << 8) | domain)
    assert [int(x) for x in w] == [o[2 * i] | (o[2 * i + 1] << 32) for i in range(8)]
    many = sr.rng_words8(keys["secret"], obj, np.array([block - 1, block]), epoch, attempt, domain)
    assert many.shape == (2, 8) and (many[1] == w).all()


def test_test_seed_expansion_is_splitmix64():
    # splitmix64's published first outputs for seed 0 (Steele, Lea, Flood 2014; Vigna's splitmix64.c): the first key word pair is the first output
    k = sr.rng_keys_from_test_seed(0)
    outs = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F, 0xF88BB8A8724C81EC]
    assert [int(k["secret"][2 * i]) | (int(k["secret"][2 * i + 1]) << 32) for i in range(4)] == outs
    assert not (k["secret"] == k["pub"]).any()


# ---- the definitions are the distributions they claim to be ---------------------------------------------------------------------------
def chi2_quantile(df, p_upper=1e-6):
    """the 1 - p_upper quantile of the chi-square law with df degrees of freedom"""
    try:
        from scipy.stats import chi2

        return float(chi2.isf(p_upper, df))
    except ImportError:   # Wilson-Hilferty: chi2_df ~ df (1 - 2/(9 df) + z sqrt(2/(9 df)))^3, z = the normal quantile (4.7534 at 1 - 10^-6)
        z = 4.753424
        return df * (1 - 2 / (9 * df) + z * math.sqrt(2 / (9 * df))) ** 3


def chi2_stat(observed, expected):
    observed, expected = np.asarray(observed, dtype=np.float64), np.asarray(expected, dtype=np.float64)
    assert expected.min() >= 5 and abs(observed.sum() - expected.sum()) < 1e-6 * expected.sum()
    return float(((observed - expected) ** 2 / expected).sum())


@pytest.fixture(scope="module")
def words():
    """2^20 words of one object of the fixed seed's secret key (2^17 blocks: within one object's 2^20)"""
    return sr.poly_words(sr.rng_keys_from_test_seed(SEED)["secret"], 3, DRAWS, 0, 0, sr.RNG_KSK_E)


def test_ternary_is_uniform_on_three_values(words):
    t = sr.ternary(words)
    assert set(np.unique(t)) == {-1, 0, 1}
    stat = chi2_stat([(t == v).sum() for v in (-1, 0, 1)], [DRAWS / 3] * 3)
    print("ternary chi-square", stat, "bound", chi2_quantile(2))
    assert stat <= chi2_quantile(2)          # quantile (2 degrees of freedom) 27.63; observed 3.36
    # the definition itself on hand-made words: the lowest group that is not 3 decides
    hand = np.array([0b00, 0b01, 0b10, 0b0011, 0b0111, 0b101111, (1 << 64) - 1, ((1 << 62) - 1) | (2 << 62)], dtype=np.uint64)
    assert list(sr.ternary(hand)) == [-1, 0, 1, -1, 0, 1, 0, 1]


def test_centred_binomial_is_binomial_42_minus_21(words):
    v = sr.cbd(words)
    assert v.min() >= -21 and v.max() <= 21
    pmf = np.array([math.comb(42, k) for k in range(43)], dtype=np.float64) / 2.0**42
    exp, obs = pmf * DRAWS, np.bincount(v + 21, minlength=43).astype(np.float64)
    keep = exp >= 5                            # the tails (expected count below 5) are merged into one cell each side
    lo, hi = int(np.argmax(keep)), 43 - int(np.argmax(keep[::-1]))
    exp_m = np.concatenate([[exp[: lo + 1].sum()], exp[lo + 1 : hi - 1], [exp[hi - 1 :].sum()]])
    obs_m = np.concatenate([[obs[: lo + 1].sum()], obs[lo + 1 : hi - 1], [obs[hi - 1 :].sum()]])
    stat, df = chi2_stat(obs_m, exp_m), len(exp_m) - 1
    print("cbd chi-square", stat, "df", df, "bound", chi2_quantile(df))
    assert stat <= chi2_quantile(df)         # quantile (28 degrees of freedom) 78.82; observed 29.81
    assert abs(v.std() - math.sqrt(10.5)) < 0.01   # sigma = sqrt(42 / 4) = 3.24
    # bits 0..20 count up, bits 21..41 count down, bits 42..63 do not count
    hand = np.array([(1 << 21) - 1, ((1 << 21) - 1) << 21, (1 << 42) - 1, ((1 << 22) - 1) << 42, 0b111 | (1 << 21), 1 << 20, 1 << 41], dtype=np.uint64)
    assert list(sr.cbd(hand)) == [21, -21, 0, 0, 2, 1, -1]


@pytest.mark.parametrize("q", [Q60, Q46])
def test_uniform_residues_are_uniform(q):
    r, retries = sr.uniform_limb(sr.rng_keys_from_test_seed(SEED)["pub"], 77, q, DRAWS, sr.RNG_KSK_A)
    assert int(r.max()) < q
    bounds = np.array([-(-k * q // 256) for k in range(257)], dtype=np.uint64)      # 256 buckets of q / 256 residues (+-1), exact integers
    obs = np.bincount(np.searchsorted(bounds, r, side="right") - 1, minlength=256)
    exp = np.diff(bounds.astype(np.float64)) / float(q) * DRAWS
    stat = chi2_stat(obs, exp)
    print(f"uniform mod {q:#x}: chi-square", stat, "bound", chi2_quantile(255), "retried", int((retries > 0).sum()))
    assert stat <= chi2_quantile(255)        # quantile (255 degrees of freedom) 377.08; observed 265.06 (60 bits) and 264.27 (46 bits)
    # a draw is rejected with probability (2^b - q) / 2^b: ~2^-34 for the 60-bit prime (none in 2^20), ~2^-18 for the 46-bit one (about 4 expected, 2 seen)
    if q == Q60:
        assert not retries.any()
    else:
        assert 1 <= int((retries > 0).sum()) <= 20 and int(retries.max()) == 1
        # a retried coefficient is the same word index of the block at attempt 1; everything else is the attempt-0 draw
        key, sh = sr.rng_keys_from_test_seed(SEED)["pub"], 64 - q.bit_length()
        w0 = sr.poly_words(key, 77, DRAWS, 0, 0, sr.RNG_KSK_A) >> np.uint64(sh)
        w1 = sr.poly_words(key, 77, DRAWS, 0, 1, sr.RNG_KSK_A) >> np.uint64(sh)
        again = retries > 0
        assert (w0[again] >= q).all() and (r[again] == w1[again]).all() and (r[~again] == w0[~again]).all()


def test_sparse_secret_has_the_weight_and_skips_occupied_positions():
    key = sr.rng_keys_from_test_seed(SEED)["secret"]
    for N, h in ((1 << 12, 32), (1 << 12, 1 << 11)):             # the second: half the ring, many collisions
        s = sr.sparse_secret(key, N, h, sr.RNG_ESK)
        assert int((s != 0).sum()) == h and set(np.unique(s)) <= {-1, 0, 1}
    w = sr.rng_words8(key, 0, 0, 0, 1, sr.RNG_SK)                  # the first word places the first coefficient
    s = sr.sparse_secret(key, 1 << 12, 1, sr.RNG_SK)
    assert s[(int(w[0]) >> 8) % (1 << 12)] == (1 if int(w[0]) & 1 else -1)


# ---- addresses never collide ---------------------------------------------------------------------------------------------------------------
def collisions(draws):
    """pairs of draws that share a ChaCha20 block under the same key and nonce; asserts that every quantity fits its field"""
    groups = defaultdict(list)
    for d in draws:
        assert 0 < d.blocks <= 1 << sr.BLOCK_BITS, d
        assert 0 <= d.obj < 1 << sr.OBJECT_BITS, d
        assert 0 <= d.attempts[0] < d.attempts[1] <= sr.ATTEMPTS, d
        assert 0 < d.domain < 256 and 0 <= d.epoch < 1 << 48, d
        groups[(d.key, d.domain, d.epoch)].append(d)
    bad = []
    for members in groups.values():
        classes = defaultdict(list)            # same (key, domain, epoch) and the same attempts: the counter ranges must be disjoint
        for d in members:
            classes[d.attempts].append(d)
        names = list(classes)
        pools = [classes[a] for a in names]
        for i, a in enumerate(names):          # two attempt ranges that intersect: their draws must be disjoint too
            for j in range(i + 1, len(names)):
                if a[0] < names[j][1] and names[j][0] < a[1]:
                    pools.append(classes[a] + classes[names[j]])
        for pool in pools:
            start = np.array([d.obj << sr.BLOCK_BITS for d in pool], dtype=np.uint64)
            end = start + np.array([d.blocks for d in pool], dtype=np.uint64)
            order = np.argsort(start, kind="stable")
            hit = np.nonzero(start[order][1:] < end[order][:-1])[0]
            bad += [(pool[order[k]].who, pool[order[k + 1]].who) for k in hit]
    return bad


# What the fields allow: a block number has 20 bits (N <= 2^23), an attempt 8, and the object of a uniform half is
# (key_id * 64 + digit) * 64 + limb -- AT MOST 64 LIMBS AND AT MOST 64 DIGITS PER KEY (Context refuses more than 64 primes; SEAL-layout keys have
# one digit fewer than primes, grouped-digit keys at most 16).  Encryptor objects count up from 0 and a plan's opcode-10 items from 2^32: at
# most 2^32 encryptions per VM and 2^12 * 2^32 = 2^44 objects before the counter's 64 bits are full.
CASES = {
    "largest geometry": dict(logN=17, limbs=40, digits=39),
    "config 3, SEAL layout": dict(logN=16, limbs=25, digits=24),
    "2^16 encryptions": dict(logN=13, limbs=7, digits=6, encryptions=[(n, n // 30000) for n in range(1 << 16)]),
    "600 opcode-10 items": dict(logN=13, limbs=7, digits=6, boot=(1, 2), encryptions=[(0, 0), (1, 0), (2, 1)],
                                plan_items=[(k, e) for e in range(3) for k in range(600)]),
}


@pytest.mark.parametrize("case", list(CASES))
def test_addresses_never_collide(case):
    kw = CASES[case]
    assert kw["limbs"] <= sr.LIMB_SLOTS and kw["digits"] <= sr.DIGIT_SLOTS
    table = list(sr.draws(**kw))
    assert len({d.who for d in table}) == len(table)
    assert collisions(table) == []
    # private and published values never come from the same key
    assert {d.key for d in table if d.domain in (sr.RNG_PK_A, sr.RNG_KSK_A)} == {"pub"}
    assert {d.key for d in table if d.domain not in (sr.RNG_PK_A, sr.RNG_KSK_A)} == {"secret"}


def test_the_limits_are_sharp():
    """one limb or one digit beyond 64 does collide (so the check above can fail), and 64 of each do not"""
    assert collisions(sr.draws(12, 64, 64, galois_elts=[3], boot=(1, 2))) == []
    assert ("relin digit 0 a limb 64", "relin digit 1 a limb 0") in collisions(sr.draws(12, 65, 64, galois_elts=[3]))
    assert ("relin digit 64 e", "swk_down digit 0 e") in collisions(sr.draws(12, 64, 65, galois_elts=[3], boot=(1, 2)))
    # Encryptor objects and a plan's opcode-10 objects meet only after 2^32 encryptions
    assert collisions(sr.draws(12, 5, 4, galois_elts=[], encryptions=[(1 << 32, 0)], plan_items=[(0, 0)])) != []
