"""GPU: noise measured on the device (dacapo_amd/noise.py): dc_poly_error_stats against the exact reference (noise_reference.py) on crafted
polynomials, hevm_phase_batch against Oracle.decrypt limb for limb, noise.op_noise against the same statistics computed from the oracle's
limbs for the same keys and inputs and against the closed forms, the reference's own rescale row, and the profile tool's table builder.
N = 2^12 unless a test says otherwise."""
import ctypes
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import noise_reference as nr  # noqa: E402
from gpu_helpers import _get_ct, _import_keys  # noqa: E402
from oracle.oracle import Ciphertext, Oracle  # noqa: E402

SEED = 0x4845564D
_RINGS: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _release_rings_after_the_module():
    yield
    _RINGS.clear()


def _ring(logN=12, K=6, primes=None):
    """a kernel-level context and the oracle on the same chain.  K = 6 for the crafted polynomials: 5 limbs AND a multiplier prime above them"""
    from dacapo_amd import lowlevel as ll

    key = (logN, K, tuple(primes or ()))
    if key not in _RINGS:
        ctx = ll.Context(logN, K, primes=primes)
        o = Oracle(logN, K, primes=primes)
        assert ctx.primes == o.primes
        _RINGS[key] = (ctx, o)
    return _RINGS[key]


# ---- dc_poly_error_stats on crafted polynomials -------------------------------------------------------------------------------------------
def _targets(o, ell, rng, big_positive=True):
    """N integers D to recover: the edges of the lifted range (-M/2, M/2), M = q0 or q0 q1, spread over several workgroups' tiles, and
    58-bit noise elsewhere.  The top of the range appears twice with + and once with -: the sum is then dominated by terms of one sign, so
    that its 1e-9 is a statement about the summation and not about cancellation."""
    N = o.N
    M = o.primes[0] if ell == 1 else o.primes[0] * o.primes[1]
    D = [int(x) for x in rng.integers(-(1 << 58), 1 << 58, N)]
    top = (M - 1) // 2
    edge = {0: 0, 1: 1, 2: -1, 3: top, 511: -top, 512: top - 1, 1023: -(top - 1), 1024: top if big_positive else 5, N - 1: -3, N - 2: 2}
    if ell >= 2:
        edge.update({700: (1 << 100) + 12345, 2049: -(1 << 100) - 7})
    for j, v in edge.items():
        D[j] = v
    return D


def _residues(o, values, ell):
    """integers -> [ell][N] NTT-form residues (the oracle's transform)"""
    coef = np.array([[v % q for v in values] for q in o.primes[:ell]], dtype=np.uint64)
    return o.ntt_fwd(coef, list(range(ell)))


def _craft(o, ell, count, with_want, lift_prime, rng, targets=None):
    """per item (got, want or None) in NTT form with m got - want == the target integers modulo every limb"""
    m = 1 if lift_prime < 0 else o.primes[lift_prime]
    items = []
    for b in range(count):
        D = targets[b] if targets is not None else _targets(o, ell, rng)
        if with_want:
            G = [int(x) for x in rng.integers(0, 1 << 59, o.N)]
            items.append((_residues(o, G, ell), _residues(o, [m * g - d for g, d in zip(G, D)], ell), D))
        elif m == 1:
            items.append((_residues(o, D, ell), None, D))
        else:  # m got with nothing subtracted: whatever integers m G lifts to
            G = [int(x) for x in rng.integers(-(1 << 50), 1 << 50, o.N)]
            items.append((_residues(o, G, ell), None, None))
    return items


def _device_stats(ctx, items, ell, lift_prime, pad_words=0):
    """the items at a stride of ell N + pad_words, through Context.error_stats"""
    from dacapo_amd import lowlevel as ll

    count, stride = len(items), ell * ctx.N + pad_words
    got = np.full((count, stride), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)  # the padding must not be read
    want = got.copy()
    for b, (g, w, _) in enumerate(items):
        got[b, : ell * ctx.N] = g.ravel()
        if w is not None:
            want[b, : ell * ctx.N] = w.ravel()
    dg = ll.DeviceBuffer.from_host(got)
    dw = ll.DeviceBuffer.from_host(want) if items[0][1] is not None else None
    return ctx.error_stats(dg, dw, ell, count, lift_prime, got_stride=stride, want_stride=stride)


def _check(o, stats, items, ell, lift_prime, inconsistent=None):
    for b, (st, (g, w, D)) in enumerate(zip(stats, items)):
        ref = nr.error_stats(o, g, w, ell, lift_prime)
        if D is not None and inconsistent is None:  # the crafted integers are what both recover
            assert ref == nr.stats_of(D, 1 if lift_prime < 0 else o.primes[lift_prime])
        assert st.max_abs == ref["max_abs"], (b, st.max_abs, ref["max_abs"])
        assert st.inconsistent == ref["inconsistent"] == (0 if inconsistent is None else inconsistent[b]), (b, st.inconsistent, ref["inconsistent"])
        assert nr.close(st.sum_sq, ref["sum_sq"]), (b, st.sum_sq, float(ref["sum_sq"]))
        assert nr.close(st.sum, ref["sum"]), (b, st.sum, float(ref["sum"]))


@pytest.mark.parametrize("ell", [1, 2, 3, 5])
def test_error_stats_equal_the_exact_reference(ell):
    """count 1 and 3 (at a stride larger than ell N), want given and NULL, multiplier 1 and a prime: max |D| and the inconsistency count ==,
    the two sums within 1e-9 (N additions of relative 2^-53 each are 5e-13 at this N; the bound leaves three orders of magnitude)"""
    ctx, o = _ring()
    rng = np.random.default_rng(40 + ell)
    for count, with_want, lift in [(1, True, -1), (3, True, 5), (3, False, -1), (1, False, 5)]:
        items = _craft(o, ell, count, with_want, lift, rng)
        _check(o, _device_stats(ctx, items, ell, lift, pad_words=2 * ctx.N if count > 1 else 0), items, ell, lift)


def test_error_stats_count_limbs_that_contradict_the_lifted_value():
    """ell = 3: 7 coefficients of item 1 hold M/2 + 5 and beyond (M = q0 q1), which three limbs represent and two cannot: the value lifted
    from limbs 0 and 1 is off by M and limb 2 says so.  Items 0 and 2 report none."""
    ctx, o = _ring()
    rng = np.random.default_rng(7)
    M = o.primes[0] * o.primes[1]
    targets = [_targets(o, 3, rng) for _ in range(3)]
    for k, j in enumerate([5, 300, 513, 1500, 2048, 3000, 4095]):
        targets[1][j] = (M - 1) // 2 + 5 + 1000 * k
    items = _craft(o, 3, 3, True, -1, rng, targets)
    stats = _device_stats(ctx, items, 3, -1, pad_words=2 * ctx.N)
    assert [s.inconsistent for s in stats] == [0, 7, 0]
    _check(o, stats, items, 3, -1, inconsistent=[0, 7, 0])


def test_error_stats_multiplier_below_the_limb_count_ignores_that_limb_of_got():
    """the form a rescale to ONE prime is measured in: got = (out, anything) over two limbs, want = the operand's two limbs, multiplier
    q_1: D = q_1 out - in is lifted from (q_1 out - in mod q_0, -in mod q_1) although it exceeds q_0 / 2"""
    ctx, o = _ring()
    rng = np.random.default_rng(8)
    q0, q1 = o.primes[0], o.primes[1]
    out = [int(x) for x in rng.integers(-(1 << 30), 1 << 30, o.N)]
    err = [int(a) * q1 + int(r) for a, r in zip(rng.integers(-40, 40, o.N), rng.integers(0, q1, o.N))]  # |D| ~ 2^65 > q_0 / 2
    g = _residues(o, out, 2)
    g[1] = rng.integers(0, q1, o.N, dtype=np.uint64)  # never read into D
    items = [(g, _residues(o, [q1 * a - d for a, d in zip(out, err)], 2), None)]
    stats = _device_stats(ctx, items, 2, 1)
    _check(o, stats, items, 2, 1)
    assert stats[0].max_abs == max(abs(d) for d in err) and nr.close(stats[0].sum, nr.stats_of(err, q1)["sum"])


def test_error_stats_at_n_8192():
    ctx, o = _ring(13, 4)
    rng = np.random.default_rng(9)
    items = _craft(o, 3, 2, True, 3, rng)
    _check(o, _device_stats(ctx, items, 3, 3, pad_words=ctx.N), items, 3, 3)


def test_error_stats_on_the_generic_width_build():
    """the chain 60, 51, 51 bits (+ a 60-bit prime above them as multiplier): q1 narrower than q0, a narrow limb checked against the lift"""
    from dacapo_amd import ckks_boot

    ctx, o = _ring(12, 4, primes=ckks_boot.mixed_prime_chain(12, [60, 51, 51, 60]))
    assert [q.bit_length() for q in ctx.primes] == [60, 51, 51, 60]
    rng = np.random.default_rng(10)
    for ell, with_want, lift in [(3, True, -1), (3, True, 3), (2, False, -1), (1, True, 3)]:
        items = _craft(o, ell, 2, with_want, lift, rng)
        _check(o, _device_stats(ctx, items, ell, lift, pad_words=ctx.N), items, ell, lift)


def test_error_stats_give_identical_bits_on_every_run():
    ctx, o = _ring()
    items = _craft(o, 3, 3, True, 5, np.random.default_rng(11))
    a, b = _device_stats(ctx, items, 3, 5, pad_words=2 * ctx.N), _device_stats(ctx, items, 3, 5, pad_words=2 * ctx.N)
    assert [bytes(x) for x in a] == [bytes(x) for x in b]


# ---- hevm_phase_batch -----------------------------------------------------------------------------------------------------------------
def _program(slots, level):
    from dacapo_amd import hevm_asm as ha

    b = ha.Builder(slots=slots, init_level=level)
    b.output(b.add_plain(b.input(np.zeros(slots)), [0.25]))
    return b.assemble()[:2]


def _oracle_of(hevm, elts=(), relin=False, ks=1):
    from dacapo_amd import lowlevel as ll

    o = Oracle(hevm.logN, hevm.K)
    if ks > 1:
        o.set_hybrid(ks)
    _import_keys(o, hevm, ll, elts=list(elts), relin=relin)
    return o


def _stream_cts(hevm, reg, streams):
    from dacapo_amd import lowlevel as ll

    out = []
    for s in streams:
        hevm.select_stream(s)
        out.append(_get_ct(hevm, ll, reg))
    hevm.select_stream(0)
    return out


def _check_phase(hevm, o, level, first, count):
    from dacapo_amd import noise

    hevm.load_mem(*_program(hevm.slots, level))
    hevm.setInputs(0, np.random.default_rng(level).uniform(-1, 1, (hevm.streams, hevm.slots)))
    got = noise.phase(hevm, 0, count, first_stream=first).to_host()
    assert got.shape == (count, level, hevm.N)
    for k, ct in enumerate(_stream_cts(hevm, 0, range(first, first + count))):
        assert ct.ell == level and (got[k] == o.decrypt(ct).data).all(), (level, first + k)
    assert not (got[0] == got[1]).all()


@pytest.mark.parametrize("level", [1, 3, 4])
def test_phase_batch_equals_the_oracles_decryption(level):
    """3 streams at N = 2^12, K = 5: every stream's c0 + c1 s == Oracle.decrypt of its limbs, all streams and a window from stream 1"""
    from dacapo_amd import runner

    hevm = runner.HEVM(seed=SEED, logN=12, num_primes=5)
    hevm.set_streams(3)
    o = _oracle_of(hevm)
    _check_phase(hevm, o, level, 0, 3)
    _check_phase(hevm, o, level, 1, 2)
    # a padded stride leaves the padding alone
    pad = noise_phase_padded(hevm, 0, 3)
    assert (pad[:, :level] == np.stack([o.decrypt(ct).data for ct in _stream_cts(hevm, 0, range(3))])).all() and not pad[:, level:].any()
    hevm.close()


def noise_phase_padded(hevm, reg, count):
    from dacapo_amd import noise

    return noise.phase(hevm, reg, count, pad_limbs=1).to_host()


@pytest.fixture(scope="module")
def key_dir(tmp_path_factory):
    from dacapo_amd import runner

    d = tmp_path_factory.mktemp("noise_keys")
    full = runner.HEVM(path=str(d / "keys"), vm_options={"logn": 12, "primes": 5})
    full.close()
    return d


def test_phase_batch_on_a_full_vm_loaded_from_a_key_directory(key_dir):
    """a full VM that no client stands beside: keys from the five files of a key directory, the secret one among them"""
    from dacapo_amd import runner

    hevm = runner.HEVM(path=str(key_dir / "keys"))
    hevm.set_streams(3)
    _check_phase(hevm, _oracle_of(hevm), 3, 0, 3)
    hevm.close()


_CHILD = """
import sys
from dacapo_amd import lowlevel as ll, runner
hevm = runner.HEVM(path=sys.argv[1], option="server")
out = ll.DeviceBuffer((1, 1, hevm.N))
hevm.lw.hevm_phase_batch(hevm.vm, 0, out.ptr, hevm.N, 0, 1)
print("returned")
"""


def test_phase_batch_without_a_secret_key_aborts_with_the_message(key_dir):
    """argument checking on the host, before any launch: a child process ends in abort()"""
    r = subprocess.run([sys.executable, "-c", _CHILD, str(key_dir / "keys")], cwd=str(ROOT), capture_output=True, text=True, timeout=120)
    assert r.returncode == -6, (r.returncode, r.stderr[-400:])
    assert "hevm_phase_batch: this VM has no secret key" in r.stderr and "returned" not in r.stdout


# ---- noise.op_noise against the oracle and the closed forms -----------------------------------------------------------------------------
SAMPLES = 8  # rescale: the standard error of the mean square over 8 x 4096 coefficients is 0.8 %, the 5 % bound six of them
_VMS: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _release_vms_after_the_module():
    yield
    _VMS.clear()


def _vm(plan=1, K=5, ks=1, **opts):
    """one seeded VM per option set at N = 2^12, with its oracle twin (key for the offset-1 hop and the relinearisation key imported)"""
    from dacapo_amd import runner

    key = (plan, K, ks, tuple(sorted(opts.items())))
    if key not in _VMS:
        hevm = runner.HEVM(seed=SEED, logN=12, num_primes=K, ks_special=ks, vm_options=dict(opts, plan=plan))
        elt = 3  # the Galois element of a left rotation by one slot
        o = _oracle_of(hevm, elts=[elt], relin=True, ks=ks)
        assert o.elt_from_step(1) == elt
        _VMS[key] = (hevm, o, elt)
    return _VMS[key]


def _vm_on_the_oracles_keys(plan, tmp_root):
    """N = 2^12, K = 5 on the key set the CPU test of the closed forms pins (tests/conftest.py oracle_mid: the oracle's, seed 0x4845564D),
    written as a SEAL key directory and loaded by the VM -- see test_op_noise_equals_the_oracles_and_the_closed_form for why the key matters"""
    from dacapo_amd import lowlevel as ll
    from dacapo_amd import runner
    from oracle import seal_format as sf

    key = ("oracle keys", plan)
    if key not in _VMS:
        if "oracle" not in _VMS:
            o = Oracle(12, 5)
            o.keygen(seed=SEED)
            keydir = tmp_root.mktemp("noise_oracle_keys") / "keys"
            keydir.mkdir()
            sf.write_key_dir(keydir, o.N, o.primes, o.pk, o.sk, o.relin, o.galois, compr=sf.COMPR_ZLIB)
            _VMS["oracle"] = (o, keydir)
        o, keydir = _VMS["oracle"]
        hevm = runner.HEVM(path=str(keydir), vm_options={"plan": plan})
        assert (hevm.logN, hevm.K) == (12, 5)
        assert (ll.read_device(hevm.lw.hevm_relin_key(hevm.vm), o.relin.shape) == o.relin).all(), "the key directory did not load limb for limb"
        _VMS[key] = (hevm, o, 3)
    return _VMS[key]


def _oracle_stats(o, op, level, elt, ins, apply_galois=None):
    """the exact reference's record for one sample: the oracle performs the op on the GPU's input limbs"""
    ph = [o.decrypt(c).data for c in ins]
    if op == "rotate":
        out = (apply_galois or o.apply_galois)(ins[0], elt)
        return nr.error_stats(o, o.decrypt(out).data, o.galois_ntt(ph[0], elt), level)
    if op == "mul":
        return nr.error_stats(o, o.decrypt(o.mul_relin(ins[0], ins[1])).data, o.poly_mul(ph[0], ph[1]), level)
    got = np.concatenate([o.decrypt(o.rescale(ins[0])).data, np.zeros((1, o.N), dtype=np.uint64)])
    return nr.error_stats(o, got, ph[0], level, lift_prime=level - 1)


def _measure_and_mirror(hevm, o, elt, op, level, loop, samples=SAMPLES, apply_galois=None):
    from dacapo_amd import noise

    refs = []

    def observe(first, count):
        regs = [_stream_cts(hevm, i, range(count)) for i in range(2 if op == "mul" else 1)]
        refs.extend(_oracle_stats(o, op, level, elt, [r[k] for r in regs], apply_galois) for k in range(count))

    r = noise.op_noise(hevm, op, level, samples, loop=loop, observe=observe)
    assert r["inconsistent"] == 0 and r["samples"] == samples == len(refs) and r["level"] == (level - 1 if op == "rescale" else level)
    for got, ref in zip(r["per_sample"], refs):
        assert ref["inconsistent"] == 0 and got["max_abs"] == ref["max_abs"]
        assert nr.close(got["sum_sq"], ref["sum_sq"]) and nr.close(got["sum"], ref["sum"]), (got, ref)
    assert nr.close(r["noise"], sum(x["sum_sq"] for x in refs) / (2 * samples))
    return r


@pytest.mark.parametrize("loop", [False, True], ids=["plan", "loop"])
@pytest.mark.parametrize("op,level", [("rotate", 1), ("rotate", 2), ("rotate", 4), ("rescale", 2), ("rescale", 4), ("mul", 1), ("mul", 2),
                                      ("mul", 4)])
def test_op_noise_equals_the_oracles_and_the_closed_form(op, level, loop, tmp_path_factory):
    """in the plan (8 streams, one run) and in the loop (plan = 0: 8 runs of one stream): every sample's record is the exact reference's on
    the oracle's limbs for the same keys and inputs; the rescale within 5 % of (N/2)(1 + h)/12, the key switches within a factor 2 of theirs.

    That factor 2 is a cap on ONE key's value around an expectation over keys, and the key matters: three quarters of the closed form is the
    digits' mean q/2 times the key noise, (q / 2P) (1 + X + ... + X^(N-1)) sum_j e_j, whose mean square over the coefficients is that of a
    random walk -- about 0.81 chi^2_1 + 0.19 of its expectation -- so measured / closed form is 0.25 + 0.75 R with R that wide: its median is
    near 0.67 (the reference's own rotate row is 0.65 - 0.8 of the closed form), it cannot fall below 0.25, and it leaves (0.5, 2) for a
    sizeable share of keys.  On the keys a seeded GPU VM generates (seed 0x4845564D) the statistics equal the oracle's as well, and the rotate
    hop at 4 primes is 0.329 of the closed form (0.673 and 0.738 at 1 and 2 primes; mul 0.711, 1.051, 0.749).  The cap is therefore asserted
    on the key set on which the CPU test asserts it (test_noise_reference.py: the oracle's keys at the suite's seed), loaded by the VM from a
    key directory; a wrong formula -- centred digits, a missing division by P -- is a factor 4 or more on any key."""
    from dacapo_amd import noise

    hevm, o, elt = _vm_on_the_oracles_keys(0 if loop else 1, tmp_path_factory)
    r = _measure_and_mirror(hevm, o, elt, op, level, loop)
    ratio = r["noise"] / noise.closed_form(op, o.primes, level, o.N, nr.secret_weight(o))
    print(f"{op} at {level} primes ({'loop' if loop else 'plan'}): noise {r['noise']:.4e}, measured / closed form = {ratio:.4f}")
    assert abs(ratio - 1.0) < 0.05 if op == "rescale" else 0.5 < ratio < 2.0


def test_rotate_noise_on_a_grouped_digit_vm_equals_the_oracles():
    """ks_special = 2 (6 primes, 4 data primes): the hop is orc_rotate_ks_hybrid's; no closed form is asserted"""
    hevm, o, elt = _vm(K=6, ks=2)
    r = _measure_and_mirror(hevm, o, elt, "rotate", 3, False, samples=3)
    print(f"grouped-digit rotate at 3 primes: noise {r['noise']:.4e}")


def test_rotate_noise_on_a_hoisting_vm_equals_the_oracles():
    """ks_hoist = 1 on SEAL-layout keys: digits before the automorphism (orc_rotate_ks_hybrid at one special prime, one prime per digit)"""
    import ctypes as C

    from oracle.oracle import _p

    hevm, o, elt = _vm(ks_hoist=1)

    def hoisted(a, e):
        c0 = o.galois_ntt(a.data[0], e)
        c1 = np.zeros_like(c0)
        o.L.orc_rotate_ks_hybrid(o.ctx, a.ell, _p(np.ascontiguousarray(a.data[1])), C.c_uint32(e), _p(o.galois[e]), _p(c0), _p(c1))
        return Ciphertext(np.stack([c0, c1]), a.scale)

    r = _measure_and_mirror(hevm, o, elt, "rotate", 3, False, samples=3, apply_galois=hoisted)
    print(f"hoisted rotate at 3 primes: noise {r['noise']:.4e}")


# ---- the reference's own row --------------------------------------------------------------------------------------------------------
def test_rescale_noise_matches_the_reference_compilers_table():
    """N = 2^15, 3 primes, the default secret, 2 samples: the rescale's noise within 6 % of each of the 13 entries of the reference's
    earth.rescale_single row (they lie within 2.9 % of N (1 + h) / 24 = 2.983e7 at h = 2N/3, ours carries 0.7 % of sampling error) and within
    3 % of the closed form at this key's h.  The rotate and mul rows are printed, not asserted: the reference's figures come from one key and
    unknown inputs, its mul row is not monotonic and its rotate row is 0.65 - 0.8 of the closed form."""
    from dacapo_amd import noise, runner

    ref = json.loads((ROOT / "tests" / "golden" / "reference_noise_table.json").read_text())["noiseTable"]
    hevm = runner.HEVM(seed=SEED, logN=15, num_primes=3)
    o = _oracle_of(hevm)
    h = nr.secret_weight(o)
    r = noise.op_noise(hevm, "rescale", 2, 2)
    assert r["inconsistent"] == 0
    row = ref["earth.rescale_single"]
    print(f"rescale at 2 primes, N = 2^15: noise {r['noise']:.4e}, closed form {noise.closed_form('rescale', o.primes, 2, o.N, h):.4e} (h = {h}), "
          f"ratios to the reference's row {[round(r['noise'] / x, 3) for x in row]}")
    assert len(row) == 13 and all(abs(r["noise"] / x - 1.0) < 0.06 for x in row)
    assert abs(r["noise"] / noise.closed_form("rescale", o.primes, 2, o.N, h) - 1.0) < 0.03
    for name, op in (("earth.rotate_single", "rotate"), ("earth.mul_double", "mul")):
        for level in (1, 2):
            x = noise.op_noise(hevm, op, level, 2)
            assert x["inconsistent"] == 0
            print(f"{op} at {level} primes, N = 2^15, 3-prime chain: noise {x['noise']:.4e}, / reference's entry {x['noise'] / ref[name][level - 1]:.3f}, "
                  f"/ closed form {x['noise'] / noise.closed_form(op, o.primes, level, o.N, h):.3f}")
    hevm.close()


# ---- the profile tool's table builder --------------------------------------------------------------------------------------------------
def test_profile_tool_builds_the_three_rows(tmp_path):
    sys.path.insert(0, str(ROOT / "tools" / "legs"))
    import profile_backend as pb

    hevm, o, _ = _vm()
    rows, detail = pb.noise_table(hevm, 3, samples=2, h=nr.secret_weight(o))
    assert set(rows) == {"earth.rotate_single", "earth.rescale_single", "earth.mul_double"}
    assert all(len(v) == 3 and all(x > 0 for x in v) for v in rows.values())
    assert rows["earth.rescale_single"][0] == rows["earth.rescale_single"][1]
    assert detail["earth.rescale_single"][0]["primes"] == 2 and detail["earth.rotate_single"][0]["primes"] == 1
    f = tmp_path / "noise_table.json"
    f.write_text(json.dumps({"noiseTable": rows, "rows": detail}, indent=1))
    back = json.loads(f.read_text())
    assert back["noiseTable"] == rows and back["rows"]["earth.mul_double"][2]["measured_over_closed_form"] > 0
