"""Drop-in boundary: the C-ABI library loads and exports every symbol include/k16.h declares, the
C++ FullProver facade keeps the reference's ABI, and both fail loudly (never fall back) without a GPU."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "keyless-zk-proofs_amd")
LIB = os.path.join(PKG, "libk16.so")
HARNESS_SRC = os.path.join(ROOT, "tests", "cpp", "fullprover_harness.cpp")


def _has_gpu():
    try:
        import k16
        c = k16.Context(0)
        c.close()
        return True
    except Exception:
        return False


def build_harness(tmp_path, testing=False):
    """The C++ program standing for the Rust crate.  testing=True links the TESTING build of the library
    (libk16_testing.so, the only one with the K16_FAULT_INJECT hooks)."""
    exe = str(tmp_path / ("fullprover_harness_testing" if testing else "fullprover_harness"))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), HARNESS_SRC,
                           "-L", PKG, "-lk16_testing" if testing else "-lk16", "-Wl,-rpath," + PKG, "-pthread", "-o", exe])
    return exe


def test_library_exports_every_declared_symbol():
    assert os.path.exists(LIB), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    hdr = open(os.path.join(ROOT, "include", "k16.h")).read()
    declared = set(re.findall(r"\b(k16_[a-z0-9_]+)\s*\(", hdr))
    import k16
    assert declared == set(k16.SYMBOLS), declared ^ set(k16.SYMBOLS)
    L = ctypes.CDLL(LIB)
    for s in sorted(declared):
        assert hasattr(L, s), s
    # C++ facade: Itanium-mangled entry points bindgen binds (rust-rapidsnark/build.rs:142-146)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    for m in ("_ZN10FullProverC1EPKc", "_ZN10FullProverD1Ev", "_ZNK10FullProver5proveEPKc",
              "_ZN14ProverResponseC1E11ProverError", "_ZN14ProverResponseD1Ev"):
        assert m in syms, m


RESULT_CHANGING_SWITCHES = (b"K16_PROBE", b"K16_LAB", b"PROBE_NO_WITNESS", b"K16_FAULT_INJECT", b"nosort", b"notail")


def test_production_library_has_no_result_changing_switches():
    """Measurement probes (stale bucket sorts, witness MSMs over one point: WRONG results on purpose) and the fault hooks
    exist only in lab / testing builds (-DK16_LAB, -DK16_TESTING).  The production library must not even contain their
    NAMES: an inherited environment variable cannot make a service return invalid proofs."""
    blob = open(LIB, "rb").read()
    for name in RESULT_CHANGING_SWITCHES:
        assert name not in blob, name
    # ... and every tuning switch it does read is read in ONE place, k16_tuning::from_env (ctx.hip), when a context is created
    src = os.path.join(PKG, "csrc")
    offenders = []
    for fn in sorted(os.listdir(src)):
        if not fn.endswith((".hip", ".inc", ".h", ".cpp")):
            continue
        for ln, line in enumerate(open(os.path.join(src, fn), errors="ignore"), 1):
            if "getenv(" in line and not line.lstrip().startswith("//"):
                offenders.append((fn, ln, line.strip()))
    allowed = {"ctx.hip", "fullprover.cpp"}        # from_env + the host pool's size; the facade's K16_DEVICE(S) / K16_LOG at construction
    lab_only = [o for o in offenders if o[0] not in allowed]
    # what is left outside those files sits behind #ifdef K16_LAB / K16_TESTING -- or belongs to the RCCL leg, which has no
    # context when it loads the library (k16_rank_comm_unique_id): K16_RCCL_LIB is read once per process, the gather's
    # time limit once per communicator; neither selects a result
    for fn, ln, line in lab_only:
        assert "K16_LAB" in line or "K16_FAULT_INJECT" in line or \
            (fn == "msm_sharded.hip" and ("K16_RCCL_LIB" in line or "K16_RANK_COMM_TIMEOUT_MS" in line)), (fn, ln, line)
    # ... and WHICH variables the production build reads is a decision, not an accident: a new switch has to be added here
    assert production_env_names(src) == ENV_ALLOWED


# Every "K16_..." name libk16.so passes to getenv (directly or through from_env's one-line helpers).  A name enters this
# list when a test uses it, a deployer is told about it (INTEGRATION.md / README.md), it is a diagnostic, or the path it
# forces is live for other inputs; a rejected experiment's switch leaves with its code (DESIGN_HISTORY.md).
ENV_ALLOWED = {
    # ctx.hip, k16_tuning::from_env
    "K16_ATOMIC_SORT", "K16_SEG", "K16_CLASSES", "K16_B_SORT", "K16_B_DERIVE", "K16_B2_FIRST", "K16_FUSED_HSCALARS",
    "K16_VERIFY_NO_COOP", "K16_VERIFY_COOP_MAX", "K16_VERIFY_COOP_TRACE", "K16_TRACE", "K16_TRACE_ENQ", "K16_TRACE_HOST",
    "K16_NO_WARMUP",
    # ctx.hip, the process's host thread pool
    "K16_HOST_THREADS", "K16_UPLOAD_THREADS",
    # fullprover.cpp, the facade's constructor
    "K16_LOG", "K16_DEVICES", "K16_DEVICE", "K16_POOL_STREAM_OFFSET",
    # msm_sharded.hip, the RCCL leg
    "K16_RCCL_LIB", "K16_RANK_COMM_TIMEOUT_MS",
}


def production_env_names(src):
    """The set of "K16_..." string literals that reach getenv in csrc/, outside #ifdef K16_LAB / K16_TESTING blocks: the
    argument of a getenv( call, or of one of the lambdas of from_env that forward their argument to it."""
    import re
    call = re.compile(r'\b(getenv|on|onv|num)\(\s*"(K16_[A-Z0-9_]+)"')
    names = set()
    for fn in sorted(os.listdir(src)):
        if not fn.endswith((".hip", ".inc", ".h", ".cpp")):
            continue
        guarded = []                       # one entry per open #if: True when it (or an enclosing one) is a lab / testing block
        for line in open(os.path.join(src, fn), errors="ignore"):
            t = line.strip()
            if t.startswith("#if"):
                lab = t.startswith("#ifdef") and ("K16_LAB" in t or "K16_TESTING" in t)
                guarded.append(lab or (bool(guarded) and guarded[-1]))
            elif t.startswith("#else") and guarded:
                guarded[-1] = len(guarded) > 1 and guarded[-2]   # the #else of a lab block is production code
            elif t.startswith("#endif") and guarded:
                guarded.pop()
            elif not (guarded and guarded[-1]) and not t.startswith("//"):
                names.update(m.group(2) for m in call.finditer(line))
    return names


def test_rccl_test_double_is_not_part_of_the_product():
    """tests/cpp/fake_rccl.cpp stands in for RCCL in tests/test_gpu_rank_comm.py only: neither the shared library, the testing
    build nor the static archive contains it, links any RCCL, or exports an nccl* symbol (RCCL is dlopen'ed at the first use)."""
    for name in ("libk16.so", "libk16_testing.so", "libk16.a"):
        path = os.path.join(PKG, name)
        assert os.path.exists(path), path
        blob = open(path, "rb").read()
        assert b"k16_fake_rccl" not in blob and b"fake rccl" not in blob, name
        if name.endswith(".so"):
            dyn = subprocess.check_output(["readelf", "-d", path]).decode()
            assert "rccl" not in dyn and "nccl" not in dyn, name
            syms = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
            assert " nccl" not in syms and "ncclAllGather" not in syms.replace("k16_", ""), name
    mk = open(os.path.join(PKG, "Makefile")).read()
    assert "fake_rccl" not in mk


@pytest.mark.gpu
def test_probe_variables_in_the_environment_do_not_change_production_results(tmp_path, toy_paths):
    """The production library under every probe / fault variable a lab shell may have left behind: proofs still equal the
    oracle's, byte for byte, and a repeated MSM over the same scalar array is sorted again (the `nosort` probe reused a
    stale sort)."""
    zkey, wtns, _ = toy_paths
    code = '''
import os, sys
sys.path[:0] = [%r, %r, %r]
import numpy as np
import k16, oracle_lib as ol, bench
from gpu_common import np_scalars
ctx = k16.Context(0)
p = k16.Prover(ctx, %r)
z = bytes(32)
assert p.prove_file(%r, z, z) == ol.prove_files(%r, %r, z, z)
p.close()
zk = bench.synth_zkey_bytes(ctx, k16, 5000, 1, 1 << 13, 20000)
open(%r, "wb").write(zk)
w = bench.synth_witness(5000, 5)
bench.write_wtns(%r, w)
p = k16.Prover(ctx, %r)
assert p.prove_mem(w, z, z) == ol.prove_files(%r, %r, z, z)
p.close()
n = 1 << 16
B = ol.gen_points(0, 0, n)
d_b = ctx.to_device(B)
for seed in (1, 2):
    S = np_scalars(seed, n, "uniform")
    d_s = ctx.to_device(S)            # the SAME device address both times (freed and allocated again) is the stale-sort case
    ctx.msm_enqueue(0, d_b, d_s, n)
    _, got = ctx.msm_finish(0)
    assert got == ol.msm(0, B, S, nthreads=4)[1], seed
    d_s.free()
print("production results unchanged")
''' % (os.path.join(ROOT, "tests"), ROOT, PKG, zkey, wtns, zkey, wtns, str(tmp_path / "s.zkey"), str(tmp_path / "s.wtns"),
       str(tmp_path / "s.zkey"), str(tmp_path / "s.zkey"), str(tmp_path / "s.wtns"))
    env = dict(os.environ, K16_PROBE="nosort,notail", K16_LAB_PROBE="nosort,notail", K16_PROBE_NO_WITNESS="1",
               K16_LAB_PROBE_NO_WITNESS="1", K16_FAULT_INJECT="hip_after_msm")
    env.pop("K16_LIB_PATH", None)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0 and "production results unchanged" in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU behaviour")
def test_no_gpu_fails_loudly_no_fallback(tmp_path, toy_paths):
    import k16
    with pytest.raises(k16.K16Error) as ei:
        k16.Context(0)
    assert ei.value.rc == -1
    zkey, wtns, _ = toy_paths
    exe = build_harness(tmp_path)
    out = subprocess.run([exe, zkey, wtns], capture_output=True, text=True, timeout=120)
    lines = out.stdout.splitlines()
    assert lines[0] == "state=1"                       # not OK
    assert lines[1].startswith("type=1 error=1")       # ERROR / PROVER_NOT_READY (fullprover.cpp:117-121)
    assert lines[2] == ""                              # raw_json = ""
    assert "no CPU fallback" in out.stderr


def test_pool_level_entry_points_refuse_a_prover_that_is_not_ready():
    """k16_fullprover_prove_mem / _compact_lease / _prove_compact / _compact_cancel on a FullProver object that is not OK (what a
    bindgen caller holds after a failed constructor: impl = NULL, state = ZKEY_FILE_LOAD_ERROR) and on null / foreign leases:
    status codes, never a crash, nothing leased.  No GPU needed: the object is never dereferenced beyond its two fields."""
    L = ctypes.CDLL(LIB)

    class Fields(ctypes.Structure):                      # include/k16_fullprover.hpp: { FullProverImpl* impl; FullProverState state; }
        _fields_ = [("impl", ctypes.c_void_p), ("state", ctypes.c_int)]

    fp = Fields(None, 1)
    lease, narrow, idx, val = ctypes.c_void_p(0x1234), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    cap, nv, ms = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_int(7)
    buf = ctypes.create_string_buffer(64)
    L.k16_fullprover_compact_lease.argtypes = [ctypes.c_void_p] + [ctypes.c_void_p] * 6
    L.k16_fullprover_prove_compact.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p]
    L.k16_fullprover_compact_cancel.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.k16_fullprover_prove_mem.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p]
    rc = L.k16_fullprover_compact_lease(ctypes.byref(fp), ctypes.byref(lease), ctypes.byref(narrow), ctypes.byref(idx), ctypes.byref(val),
                                        ctypes.byref(cap), ctypes.byref(nv))
    assert rc == -1 and lease.value is None              # K16_ERR_NO_DEVICE = PROVER_NOT_READY, and no lease handed out
    assert L.k16_fullprover_compact_lease(None, ctypes.byref(lease), ctypes.byref(narrow), ctypes.byref(idx), ctypes.byref(val),
                                          ctypes.byref(cap), ctypes.byref(nv)) == -1
    assert L.k16_fullprover_compact_lease(ctypes.byref(fp), None, None, None, None, None, None) == -3
    assert L.k16_fullprover_prove_compact(ctypes.byref(fp), ctypes.c_void_p(0x1234), 0, buf, 64, ctypes.byref(ms)) == -3 and ms.value == 0
    assert L.k16_fullprover_prove_compact(ctypes.byref(fp), None, 0, buf, 64, None) == -3
    assert L.k16_fullprover_compact_cancel(ctypes.byref(fp), ctypes.c_void_p(0x1234)) == -3
    wit = (ctypes.c_uint8 * 64)()
    assert L.k16_fullprover_prove_mem(ctypes.byref(fp), wit, 2, buf, 64, ctypes.byref(ms)) == -1


def test_product_never_imports_the_oracle():
    """The oracle is test infrastructure: nothing under keyless-zk-proofs_amd/ or include/ may reference it."""
    bad = []
    for base in (PKG, os.path.join(ROOT, "include")):
        for dp, _, fns in os.walk(base):
            for fn in fns:
                if fn.endswith((".so", ".o", ".pyc")):
                    continue
                txt = open(os.path.join(dp, fn), errors="ignore").read()
                if re.search(r"oracle_lib|liboracle|oracle/|bn254_ref|ora_[a-z]+\(", txt):
                    bad.append(os.path.join(dp, fn))
    assert not bad, bad


@pytest.mark.gpu
def test_fullprover_facade_on_gpu(tmp_path, toy_paths):
    import json
    import bn254_pairing as bp
    zkey, wtns, vk = toy_paths
    exe = build_harness(tmp_path)
    out = subprocess.run([exe, zkey, wtns, "3"], capture_output=True, text=True, timeout=300)
    lines = out.stdout.splitlines()
    assert lines[0] == "state=0", out.stderr
    proofs = []
    for k in range(3):
        assert lines[1 + 2 * k].startswith("type=0 error=0 ms="), lines
        proofs.append(lines[2 + 2 * k])
    assert len(set(proofs)) == 3                      # fresh CSPRNG blinding each time
    for js in proofs:
        assert json.loads(js)["protocol"] == "groth16"
        assert bp.verify_json(vk, js, [2])            # reference criterion: prover_handler.rs:279-290
    # error mapping (fullprover.cpp:91-100, 117-121, 216-221)
    missing = subprocess.run([exe, str(tmp_path / "nope.zkey"), wtns], capture_output=True, text=True, timeout=120)
    assert missing.stdout.splitlines()[0] == "state=1"          # ZKEY_FILE_LOAD_ERROR
    assert missing.stdout.splitlines()[1].startswith("type=1 error=1")
    wrong = subprocess.run([exe, wtns, wtns], capture_output=True, text=True, timeout=120)
    assert wrong.stdout.splitlines()[0] == "state=2"            # UNSUPPORTED_ZKEY_CURVE (wrong container type)
    garbage = tmp_path / "bad.wtns"
    garbage.write_bytes(b"wtns" + b"\x02\0\0\0" + b"\x01\0\0\0" + b"\xff" * 20)
    bad = subprocess.run([exe, zkey, str(garbage)], capture_output=True, text=True, timeout=120)
    assert bad.stdout.splitlines()[1].startswith("type=1 error=2")  # INVALID_INPUT
    # a witness over another prime -> WITNESS_GENERATION_INVALID_CURVE
    w = bytearray(open(wtns, "rb").read())
    i = w.index(bytes.fromhex("010000f093f5e143"))
    w[i] ^= 0x02
    other = tmp_path / "othercurve.wtns"
    other.write_bytes(bytes(w))
    oc = subprocess.run([exe, zkey, str(other)], capture_output=True, text=True, timeout=120)
    assert oc.stdout.splitlines()[1].startswith("type=1 error=3")


@pytest.mark.gpu
def test_static_archive_links_and_proves(tmp_path, toy_paths):
    """libk16.a linked the way the reference links librapidsnark.a (build.rs:61-64): whole archive + the HIP runtime, no
    libk16.so anywhere on the path; the toy proof through the C++ facade verifies as from the shared library."""
    zkey, wtns, vk = toy_paths
    arch = os.path.join(PKG, "libk16.a")
    assert os.path.exists(arch), "make libk16.a"
    exe = str(tmp_path / "harness_static")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), HARNESS_SRC,
                           "-Wl,--whole-archive", arch, "-Wl,--no-whole-archive", "-L", "/opt/rocm/lib", "-lamdhip64", "-ldl",
                           "-pthread", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    ldd = subprocess.check_output(["ldd", exe]).decode()
    assert "libk16" not in ldd
    out = subprocess.run([exe, zkey, wtns], capture_output=True, text=True, timeout=300)
    lines = out.stdout.splitlines()
    assert lines[0] == "state=0" and lines[1].startswith("type=0 error=0"), out.stdout + out.stderr
    import bn254_pairing as bp
    assert json.loads(lines[2])["protocol"] == "groth16"
    assert bp.verify_json(vk, lines[2], [2])          # reference criterion: prover_handler.rs:279-290


@pytest.mark.gpu
def test_proofs_through_the_generic_sort_and_its_dropped_masks(tmp_path):
    """the prover always hands its zero-row masks to the bucket sort; on the paths that do not implement a mask
    (the generic sort every key with more than 2^24 wires takes -- forced here with K16_ATOMIC_SORT) the mask is DROPPED,
    not refused: proofs equal the oracle's."""
    code = '''
import os, sys
sys.path[:0] = [%r, %r, %r]
import k16, oracle_lib as ol, bench
ctx = k16.Context(0)
n_vars = 140000                     # >= 2^17: the masks, the accumulation skip and B's (0,0) rows are all in play
zk = bench.synth_zkey_bytes(ctx, k16, n_vars, 1, 1 << 17, 300000)
open(%r, "wb").write(zk)
w = bench.synth_witness(n_vars, 9)
bench.write_wtns(%r, w)
z = bytes(32)
p = k16.Prover(ctx, %r)
assert p.prove_mem(w, z, z) == ol.prove_files(%r, %r, z, z, nthreads=os.cpu_count() or 8)
p.close()
print("masked proofs OK")
''' % (os.path.join(ROOT, "tests"), ROOT, PKG, str(tmp_path / "m.zkey"), str(tmp_path / "m.wtns"), str(tmp_path / "m.zkey"),
       str(tmp_path / "m.zkey"), str(tmp_path / "m.wtns"))
    for extra in ({"K16_ATOMIC_SORT": "1"},):
        env = dict(os.environ, **extra)
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, env=env)
        assert out.returncode == 0 and "masked proofs OK" in out.stdout, (extra, out.stdout[-1500:] + out.stderr[-3000:])


@pytest.mark.gpu
def test_fullprover_pool_concurrent_callers(tmp_path, toy_paths):
    """K16_DEVICES puts several provers behind ONE FullProver; concurrent prove() calls are safe and
    every proof verifies.  Here three provers share GPU 0 (a multi-GPU node lists 0,1,...,7)."""
    import json
    import bn254_pairing as bp
    zkey, wtns, vk = toy_paths
    exe = build_harness(tmp_path)
    env = dict(os.environ, K16_DEVICES="0,0,0")
    out = subprocess.run([exe, zkey, wtns, "2", "4"], capture_output=True, text=True, timeout=300, env=env)
    lines = out.stdout.splitlines()
    assert lines[0] == "state=0", out.stderr
    proofs = [lines[2 + 2 * k] for k in range(8)]      # 4 threads x 2 proofs
    for k in range(8):
        assert lines[1 + 2 * k].startswith("type=0 error=0 ms="), lines
    assert len(set(proofs)) == 8
    for js in proofs[:4]:
        assert json.loads(js)["protocol"] == "groth16"
        assert bp.verify_json(vk, js, [2])
    # a pool that names a device that does not exist fails in the constructor, loudly
    bad = subprocess.run([exe, zkey, wtns], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, K16_DEVICES="0,99"))
    assert bad.stdout.splitlines()[0] == "state=1"
    assert "no usable" in bad.stderr


@pytest.mark.gpu
def test_fullprover_pool_with_the_witness_in_memory(tmp_path, toy_paths):
    """k16_fullprover_prove_mem: the facade's pool (K16_DEVICES=0,0,0), four caller threads, the witness handed over in
    memory instead of as a file path -- what a multi-GPU service binds.  Every proof verifies
    (prover_handler.rs:279-290); a prover that failed to construct answers PROVER_NOT_READY; a witness shorter than the
    circuit is the caller's fault."""
    import json
    import bn254_pairing as bp
    zkey, wtns, vk = toy_paths
    exe = build_harness(tmp_path)
    env = dict(os.environ, K16_DEVICES="0,0,0", K16_HARNESS_MEM="1")
    out = subprocess.run([exe, zkey, wtns, "2", "4"], capture_output=True, text=True, timeout=300, env=env)
    lines = out.stdout.splitlines()
    assert lines[0] == "state=0", out.stderr
    proofs = [lines[2 + 2 * k] for k in range(8)]
    for k in range(8):
        assert lines[1 + 2 * k].startswith("type=0 error=0 ms="), lines
    assert len(set(proofs)) == 8
    for js in proofs[:4]:
        assert json.loads(js)["protocol"] == "groth16"
        assert bp.verify_json(vk, js, [2])
    missing = subprocess.run([exe, str(tmp_path / "nope.zkey"), wtns], capture_output=True, text=True, timeout=120, env=env)
    assert missing.stdout.splitlines()[0] == "state=1"
    assert missing.stdout.splitlines()[1].startswith("type=1 error=1")      # PROVER_NOT_READY
    w = open(wtns, "rb").read()
    short = tmp_path / "short.wtns"                                            # section 2 cut to two values
    i = w.index(b"\x02\x00\x00\x00", 12 + 12 + 40)
    short.write_bytes(w[:i] + b"\x02\x00\x00\x00" + (64).to_bytes(8, "little") + w[i + 12:i + 12 + 64])
    bad = subprocess.run([exe, zkey, str(short)], capture_output=True, text=True, timeout=120, env=env)
    assert bad.stdout.splitlines()[1].startswith("type=1 error=2"), bad.stdout   # INVALID_INPUT


@pytest.mark.gpu
def test_fullprover_device_fault_is_not_the_callers_fault(tmp_path, toy_paths):
    """A HIP failure inside prove() (injected: K16_FAULT_INJECT) is reported as PROVER_NOT_READY -- the class the service
    retries -- not INVALID_INPUT, the slot is rebuilt in a fresh context before it is handed out again, and the proofs
    after it are good (RS/fullprover.cpp:91-125 maps only its own exception classes; a GPU build adds this one)."""
    import json
    import bn254_pairing as bp
    zkey, wtns, vk = toy_paths
    exe = build_harness(tmp_path, testing=True)
    env = dict(os.environ, K16_FAULT_INJECT="hip_after_msm:2")
    out = subprocess.run([exe, zkey, wtns, "4"], capture_output=True, text=True, timeout=300, env=env)
    lines = out.stdout.splitlines()
    assert lines[0] == "state=0", out.stderr
    assert lines[1].startswith("type=0 error=0")
    assert lines[3].startswith("type=1 error=1"), lines           # ERROR / PROVER_NOT_READY
    assert lines[4] == ""
    for k in (5, 7):
        assert lines[k].startswith("type=0 error=0"), lines
        assert json.loads(lines[k + 1])["protocol"] == "groth16"
        assert bp.verify_json(vk, lines[k + 1], [2])


@pytest.mark.gpu
def test_fullprover_exception_in_prove_releases_the_slot(tmp_path, toy_paths):
    """An exception inside a proof (injected std::bad_alloc, testing build) ends at the C ABI's firewall as
    K16_ERR_NOMEM -> PROVER_NOT_READY, and the ONE slot of the default pool is given back: the next prove() succeeds
    instead of waiting for ever in acquire() (round-2 advisor finding).  The production build ignores the variable."""
    import json
    import bn254_pairing as bp
    zkey, wtns, vk = toy_paths
    exe = build_harness(tmp_path, testing=True)
    env = dict(os.environ, K16_FAULT_INJECT="bad_alloc_in_prove:2")
    env.pop("K16_DEVICES", None)
    out = subprocess.run([exe, zkey, wtns, "4"], capture_output=True, text=True, timeout=120, env=env)
    lines = out.stdout.splitlines()
    assert lines[0] == "state=0", out.stderr
    assert lines[1].startswith("type=0 error=0")
    assert lines[3].startswith("type=1 error=1"), lines           # ERROR / PROVER_NOT_READY
    assert lines[4] == ""
    for k in (5, 7):                                              # the pool's only slot is alive and proves correctly
        assert lines[k].startswith("type=0 error=0"), lines
        assert bp.verify_json(vk, lines[k + 1], [2])
    prod = build_harness(tmp_path)
    out = subprocess.run([prod, zkey, wtns, "3"], capture_output=True, text=True, timeout=120,
                         env=dict(env, K16_FAULT_INJECT="hip_after_msm"))
    lines = out.stdout.splitlines()
    assert [lines[1 + 2 * k].startswith("type=0 error=0") for k in range(3)] == [True] * 3, lines


@pytest.mark.gpu
def test_fullprover_pool_over_all_devices(tmp_path, toy_paths):
    """K16_DEVICES=all builds the pool from the device count (one resident key per GPU); with two or more GPUs the
    concurrent callers really prove on different ordinals (K16_LOG names the device of every proof)."""
    import bn254_pairing as bp
    import k16
    zkey, wtns, vk = toy_paths
    exe = build_harness(tmp_path)
    n_dev = k16.load().k16_device_count()
    assert n_dev >= 1
    env = dict(os.environ, K16_DEVICES="all", K16_LOG="1")
    out = subprocess.run([exe, zkey, wtns, "3", str(2 * n_dev)], capture_output=True, text=True, timeout=300, env=env)
    lines = [l for l in out.stdout.splitlines() if not l.startswith('{"timestamp"')]   # the log lines (K16_LOG=1)
    assert lines[0] == "state=0", out.stderr
    n = 3 * 2 * n_dev
    for k in range(n):
        assert lines[1 + 2 * k].startswith("type=0 error=0"), lines
    assert bp.verify_json(vk, lines[2], [2])
    used = set(re.findall(r"on device (\d+)", out.stdout))
    assert used == {str(d) for d in range(n_dev)}, (used, n_dev)
    if n_dev < 2:
        pytest.skip("one GPU here: the two-ordinal leg needs a multi-GPU node (the pool over all = [0] was exercised)")
