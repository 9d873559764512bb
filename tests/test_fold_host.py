"""CPU: the yardstick and the host-side parts of folded batch verification (k16_verify_batch_folded).

* tests/fold_reference.py, which the GPU tests compare against: the fold's value is 1 for valid proofs, not 1 with a wrong
  proof, 1 again for two cancelling errors under EQUAL weights (why the weights must be random) and not 1 under random ones;
* the recorded final-exponentiation program (csrc/verify_script.h, coop_build_finalexp_program) executed by the host
  interpreter equals final_exponentiation of the straight-line code (tests/cpp/fold_script_check.cpp);
* the two entry points are declared, listed and exported."""
import ctypes
import os
import re
import subprocess

import fold_reference as fr
import pymodel as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "keyless-zk-proofs_amd")


def _weights(seed, n):
    rng = pm.SplitMix64(seed)
    return [(rng.next() | (rng.next() << 64)) or 1 for _ in range(n)]


def test_reference_fold_value_is_one_exactly_for_valid_batches():
    vk, t = fr.build_key(3, seed=11)
    rng = pm.SplitMix64(5)
    inputs = [[rng.below(pm.R), rng.below(pm.R)] for _ in range(6)]
    w = _weights(7, 6)
    assert all(0 < x < 1 << 128 for x in w) and len(set(w)) == 6
    good = fr.make_proofs(t, inputs, seed=3)
    assert fr.fold_value(vk, good, inputs, w) == fr.GT_ONE
    one_bad = fr.make_proofs(t, inputs, seed=3, c_shift={2: 1})
    assert fr.fold_value(vk, one_bad, inputs, w) != fr.GT_ONE
    # two errors that cancel in an UNWEIGHTED sum: C_1 + 5G, C_4 - 5G
    pair = fr.make_proofs(t, inputs, seed=3, c_shift={1: 5, 4: -5})
    assert fr.fold_value(vk, pair, inputs, [1] * 6) == fr.GT_ONE
    assert fr.fold_value(vk, pair, inputs, [9] * 6) == fr.GT_ONE
    assert fr.fold_value(vk, pair, inputs, w) != fr.GT_ONE


def test_final_exponentiation_program_on_host_equals_straight_line_code(tmp_path):
    exe = str(tmp_path / "fsc")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-I", os.path.join(PKG, "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "fold_script_check.cpp"), "-o", exe], stderr=subprocess.DEVNULL)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("final exponentiation identical") == 5
    m = re.search(r"fold program: (\d+) steps .*slots (\d+) \(constants (\d+), inputs 12\)", out.stdout)
    assert m, out.stdout
    assert 0 < int(m.group(1)) and int(m.group(3)) < int(m.group(2)) < (1 << 14)


def test_fold_entry_points_are_declared_listed_and_exported():
    import k16
    hdr = open(os.path.join(ROOT, "include", "k16.h")).read()
    declared = set(re.findall(r"\b(k16_[a-z0-9_]+)\s*\(", hdr))
    lib = os.path.join(PKG, "libk16.so")
    assert os.path.exists(lib), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    L = ctypes.CDLL(lib)
    for s in ("k16_verify_batch_folded", "k16_verify_fold_gt"):
        assert s in declared, s
        assert s in k16.SYMBOLS, s
        assert hasattr(L, s), s
    m = re.search(r"#define\s+K16_VERIFY_FOLD_MIN\s+(\d+)", hdr)
    assert m and int(m.group(1)) == k16.VERIFY_FOLD_MIN
