"""Batched encrypt / decrypt (hevm_encrypt_batch / hevm_decrypt_batch / hevm_decrypt_result_batch; HEVM.setInputs / getOutputs): all streams'
inputs and results as one launch sequence must be, limb for limb and double for double, what the sequential calls give -- the randomness
included -- from host and from device memory, on SEAL-layout, grouped-digit and mixed-chain VMs, on a client VM, and across a chunk
boundary."""
import ctypes
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
from gpu_helpers import _get_ct  # noqa: E402

SEED = 0x4845564D
IO_CHUNK = 32  # streams per chunk of a batch call at these sizes (csrc/hevm_vm.hpp HEVM::kIoChunk)


def _program(slots, level):
    """one input at `level`, one result (input + 1/4)"""
    from dacapo_amd import hevm_asm as ha

    b = ha.Builder(slots=slots, init_level=level)
    b.output(b.add_plain(b.input(np.zeros(slots)), [0.25]))
    return b.assemble()[:2]


def _vm(streams, level, logN=12, num_primes=4, **kw):
    from dacapo_amd import runner

    hevm = runner.HEVM(seed=SEED, logN=logN, num_primes=num_primes, **kw)
    hevm.set_streams(streams)
    hevm.load_mem(*_program(hevm.slots, level))
    return hevm


def _limbs(hevm, reg, streams):
    """register `reg` of every listed stream as (level, scale, limbs); the selected stream is put back"""
    from dacapo_amd import lowlevel as ll

    out = []
    for s in streams:
        hevm.select_stream(s)
        c = _get_ct(hevm, ll, reg)
        out.append((c.ell, c.scale, c.data))
    hevm.select_stream(0)
    return out


def _same(a, b):
    return len(a) == len(b) and all(x[0] == y[0] and x[1] == y[1] and (x[2] == y[2]).all() for x, y in zip(a, b))


def _set_sequential(hevm, data, first):
    for k, row in enumerate(data):
        hevm.select_stream(first + k)
        hevm.setInput(0, row)
    hevm.select_stream(0)


def _decrypt_sequential(hevm, reg, streams):
    out = np.zeros((len(streams), hevm.slots))
    for k, s in enumerate(streams):
        hevm.select_stream(s)
        hevm.lw.decrypt(hevm.vm, reg, out[k].ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    hevm.select_stream(0)
    return out


def _decrypt_batch(hevm, reg, first, count):
    out = np.zeros((count, hevm.slots))
    hevm.lw.hevm_decrypt_batch(hevm.vm, reg, out.ctypes.data_as(ctypes.c_void_p), hevm.slots, first, count, 0)
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check_encrypt_equals_sequential(make_vm, level, length, first, count, streams=3):
    """VM A: select_stream + setInput per stream; VM B (same seed): one setInputs.  Register 0 of every stream is == , and so is one more
    sequential encryption on both (the batch left the encryption counter where `count` calls leave it)."""
    a, b = make_vm(streams, level), make_vm(streams, level)
    data = np.random.default_rng(5).uniform(-1, 1, (count, length))
    which = list(range(first, first + count))
    _set_sequential(a, data, first)
    b.select_stream(streams - 1)
    sel = b.getCtxt(0).data
    b.setInputs(0, data, first_stream=first)
    assert b.getCtxt(0).data == sel  # the selected stream stays
    la, lb = _limbs(a, 0, which), _limbs(b, 0, which)
    assert all(x[0] == level for x in lb) and _same(la, lb)
    assert not (lb[0][2] == lb[1][2]).all()  # ... and the streams differ
    extra = np.random.default_rng(6).uniform(-1, 1, (1, length))
    _set_sequential(a, extra, first)
    _set_sequential(b, extra, first)
    assert _same(_limbs(a, 0, [first]), _limbs(b, 0, [first]))
    return a, b


@pytest.mark.parametrize("level,length,first,count", [(3, 2048, 0, 3), (1, 100, 0, 3), (3, 100, 1, 2), (2, 7, 1, 2)])
def test_encrypt_batch_equals_sequential(level, length, first, count):
    """logN 12, 4 primes: at the top level K - 1 (the dropped prime is the special one), at level 1, with a length that does not divide the
    slot count, and on a sub-range of the streams"""
    _check_encrypt_equals_sequential(_vm, level, length, first, count)


def test_reference_parameters_take_the_large_launch_forms():
    """N = 2^15, 14 primes, level 13: the widest tile geometry and the single-crossing transform -- the launch forms of the fed regime -- give
    the sequential limbs and doubles too"""
    a, b = _check_encrypt_equals_sequential(lambda s, lv: _vm(s, lv, logN=15, num_primes=14), 13, 1 << 14, 0, 2, streams=2)
    got = _decrypt_batch(b, 0, 0, 2)
    assert (_bits(got) == _bits(_decrypt_sequential(a, 0, range(2)))).all()


def test_encrypt_batch_both_zero_encryption_forms_give_the_sequential_limbs():
    """option zenc_head = 0 (Encryptor::encrypt's sequence, batched) against the sequential calls too"""
    _check_encrypt_equals_sequential(lambda s, lv: _vm(s, lv, vm_options={"zenc_head": 0}), 3, 100, 0, 3)


def test_encrypt_batch_honours_the_zero_encryption_hook():
    a, b = _vm(3, 3), _vm(3, 3)
    for h in (a, b):
        h.lw.hevm_test_zero_encryption(h.vm, True)
    data = np.random.default_rng(7).uniform(-1, 1, (3, 100))
    _set_sequential(a, data, 0)
    b.setInputs(0, data)
    la, lb = _limbs(a, 0, range(3)), _limbs(b, 0, range(3))
    assert _same(la, lb)
    for lvl, _, limbs in lb:  # (plaintext, 0)
        assert lvl == 3 and not limbs[1].any() and limbs[0].any()


def test_decrypt_batch_equals_sequential_after_a_run():
    """3 streams of the Sobel filter at logN 13 / 7 primes: getOutputs() is the stack of the per-stream getOutput() bit for bit, and every
    stream is its own expected plaintext"""
    from dacapo_amd import hevm_asm as ha
    from dacapo_amd import runner

    hevm = runner.HEVM(seed=SEED, logN=13, num_primes=7)
    hevm.set_streams(3)
    rng = np.random.default_rng(11)
    imgs = [rng.uniform(0, 1, 4096) for _ in range(3)]
    builders = [ha.sobel_filter(im, slots=hevm.slots, init_level=6) for im in imgs]
    cst, hv, _ = builders[0].assemble()
    hevm.load_mem(cst, hv)
    _set_sequential(hevm, imgs, 0)
    hevm.run()
    want = []
    for s in range(3):
        hevm.select_stream(s)
        want.append(hevm.getOutput())
    hevm.select_stream(0)
    got = hevm.getOutputs()
    assert got.shape == (3, hevm.reslen, hevm.slots)
    assert (_bits(got) == _bits(np.stack(want))).all()
    assert (_bits(hevm.getOutputs(first_stream=1, count=2)) == _bits(np.stack(want[1:]))).all()
    for s in range(3):
        ref = builders[s].expected()[0]
        assert np.sqrt(np.mean((got[s, 0] - ref) ** 2)) < 1e-4 * max(1.0, np.abs(ref).max())


def _device_path_body(torch):
    host, dev = _vm(3, 3), _vm(3, 3)
    data = np.random.default_rng(8).uniform(-1, 1, (3, 100))
    host.setInputs(0, data)
    dev.setInputs(0, torch.tensor(data, dtype=torch.float64, device="cuda"))
    assert _same(_limbs(host, 0, range(3)), _limbs(dev, 0, range(3)))
    dev.run()
    want = dev.getOutputs()
    out = torch.zeros((3, dev.reslen, dev.slots), dtype=torch.float64, device="cuda")
    assert dev.getOutputs(out=out) is out
    assert (_bits(out.cpu().numpy()) == _bits(want)).all()
    assert np.abs(want[:, 0, :100] - (data + 0.25)).max() < 1e-4


_DEVICE_CHILD = """
import sys
import torch  # before the library: the process then runs on ONE HIP runtime, the one torch ships
if not torch.cuda.is_available():
    print("NO_TORCH_GPU")
    sys.exit(0)
sys.path.insert(0, sys.argv[1])
import test_gpu_io_batch as T
T._device_path_body(torch)
print("DEVICE_PATH_OK")
"""


def test_device_resident_inputs_and_outputs():
    """a float64 tensor on the GPU in, a float64 tensor on the GPU out: the limbs and the doubles of the host path.  In a child process that
    imports torch FIRST: torch ships a HIP runtime of its own, and in a process where the library has already loaded the system's (any
    earlier GPU test) torch finds no device."""
    pytest.importorskip("torch")
    r = subprocess.run([sys.executable, "-c", _DEVICE_CHILD, str(Path(__file__).resolve().parent)], cwd=str(ROOT), capture_output=True, text=True,
                       timeout=300)
    if "NO_TORCH_GPU" in r.stdout:
        pytest.skip("torch.cuda.is_available() is false: the device path needs a tensor in HBM")
    assert r.returncode == 0 and "DEVICE_PATH_OK" in r.stdout, (r.returncode, r.stdout[-400:], r.stderr[-1200:])


def test_launches_do_not_grow_with_count_and_chunks_keep_the_limbs():
    a, b = _vm(IO_CHUNK + 1, 3), _vm(IO_CHUNK + 1, 3)
    data = np.random.default_rng(9).uniform(-1, 1, (IO_CHUNK + 1, 100))
    b.setInputs(0, data[:1])
    one = b.io_stats()
    b.setInputs(0, data[:3])
    three = b.io_stats()
    assert one["launches"] == three["launches"] > 0 and one["chunks"] == three["chunks"] == 1
    per_chunk = three["launches"]
    _decrypt_batch(b, 0, 0, 1)
    one = b.io_stats()
    _decrypt_batch(b, 0, 0, 3)
    three = b.io_stats()
    assert one["launches"] == three["launches"] > 0 and one["chunks"] == three["chunks"] == 1
    # one above the chunk size: two chunks, the sequential limbs (4 encryptions were made above: the same number on the other VM)
    _set_sequential(a, data[:4], 0)
    _set_sequential(a, data, 0)
    b.setInputs(0, data)
    assert b.io_stats() == {"launches": 2 * per_chunk, "chunks": 2}
    every = range(IO_CHUNK + 1)
    assert _same(_limbs(a, 0, every), _limbs(b, 0, every))
    got = _decrypt_batch(b, 0, 0, IO_CHUNK + 1)
    assert b.io_stats()["chunks"] == 2
    assert (_bits(got) == _bits(_decrypt_sequential(b, 0, every))).all()


def _check_other_context(make_vm, level):
    a, b = _check_encrypt_equals_sequential(make_vm, level, 100, 0, 2, streams=2)
    got = _decrypt_batch(b, 0, 0, 2)
    assert (_bits(got) == _bits(_decrypt_sequential(b, 0, range(2)))).all()
    assert (_bits(got) == _bits(_decrypt_sequential(a, 0, range(2)))).all()  # (same limbs, same key)
    return got


def test_grouped_digit_vm():
    """logN 12, 6 primes of which 2 special: the top level's dropped prime is the first special one"""
    got = _check_other_context(lambda s, lv: _vm(s, lv, num_primes=6, ks_special=2), 4)
    assert np.isfinite(got).all()
    _check_other_context(lambda s, lv: _vm(s, lv, num_primes=6, ks_special=2), 2)


def test_mixed_chain_on_the_generic_width_build():
    from dacapo_amd import ckks_boot

    chain = ckks_boot.mixed_prime_chain(12, [60, 51, 51, 60])
    _check_other_context(lambda s, lv: _vm(s, lv, num_primes=0, primes=chain), 3)
    _check_other_context(lambda s, lv: _vm(s, lv, num_primes=0, primes=chain), 1)


@pytest.fixture(scope="module")
def key_dir(tmp_path_factory):
    """a key directory written by a full VM at logN 12 / 4 primes, with a one-input program next to it"""
    from dacapo_amd import runner

    d = tmp_path_factory.mktemp("io_batch_keys")
    full = runner.HEVM(path=str(d / "keys"), vm_options={"logn": 12, "primes": 4})
    cst, hv = _program(full.slots, 3)
    (d / "_hecate_t.cst").write_bytes(cst)
    (d / "t.40._hecate_t.hevm").write_bytes(hv)
    full.close()
    return d


def test_client_vm_encrypts_and_decrypts_batches(key_dir, tmp_path):
    from dacapo_amd import runner

    cst, prog = str(key_dir / "_hecate_t.cst"), str(key_dir / "t.40._hecate_t.hevm")
    full = runner.HEVM(path=str(key_dir / "keys"))
    client = runner.HEVM(path=str(key_dir / "keys"), option="client")
    for h in (full, client):
        h.set_streams(2)
        h.load(cst, prog)
    data = np.random.default_rng(10).uniform(-1, 1, (2, 100))
    want = np.stack([np.resize(row, full.slots) for row in data])  # src[i % len]

    def move(src, dst):
        for s in range(2):
            src.select_stream(s)
            dst.select_stream(s)
            src.saveCtxt(0, tmp_path / f"ct{s}.seal")
            dst.loadCtxt(0, tmp_path / f"ct{s}.seal")
        src.select_stream(0)
        dst.select_stream(0)

    client.setInputs(0, data)
    move(client, full)
    got = _decrypt_sequential(full, 0, range(2))
    assert np.sqrt(np.mean((got - want) ** 2)) < 1e-4
    full.setInputs(0, -data)
    move(full, client)
    got = _decrypt_batch(client, 0, 0, 2)
    assert np.sqrt(np.mean((got + want) ** 2)) < 1e-4


_CHILD = """
import ctypes, sys
import numpy as np
from dacapo_amd import runner
keys, case = sys.argv[1], sys.argv[2]
data = np.zeros((2, 8))
ptr = data.ctypes.data_as(ctypes.c_void_p)
if case == "streams":
    hevm = runner.HEVM(path=keys)
    hevm.set_streams(2)
    hevm.lw.hevm_encrypt_batch(hevm.vm, 0, ptr, 8, 8, 1, 2, 0)
else:
    hevm = runner.HEVM(path=keys, option="server")
    hevm.lw.hevm_encrypt_batch(hevm.vm, 0, ptr, 8, 8, 0, 1, 0)
print("returned")
"""


@pytest.mark.parametrize("case,message", [("streams", "hevm_encrypt_batch: streams 1..2 outside 0..1"),
                                          ("server", "hevm_encrypt_batch: this VM has no public key")])
def test_bad_arguments_abort_with_the_documented_message(key_dir, case, message):
    """argument checking on the host, before any launch: a child process (that has launched nothing itself) ends in abort()"""
    r = subprocess.run([sys.executable, "-c", _CHILD, str(key_dir / "keys"), case], cwd=str(ROOT), capture_output=True, text=True, timeout=120)
    assert r.returncode == -6, (r.returncode, r.stderr[-400:])
    assert message in r.stderr and "returned" not in r.stdout
