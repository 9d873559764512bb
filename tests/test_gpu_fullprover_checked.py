"""-m gpu : checked proving behind the drop-in FullProver (include/k16.h k16_fullprover_set_r1cs, k16_fullprover_last_rejection)
through tests/cpp/fullprover_checked_harness.cpp, a child process with a K16_DEVICES=0,0 pool on a small set-up key: four
threads prove good and differently broken witnesses at once, through k16_fullprover_prove_mem and FullProver::prove;
every thread's rejection is its own witness's list from the reference checker of tests/r1cs_builder.py."""
import os
import subprocess

import pytest

import pymodel as pm
import r1cs_builder as rb
import setup_reference as sr
import valid_key_builder as vkb

pytestmark = pytest.mark.gpu

R = pm.R
ERR_FORMAT = -5
NONE, BROKEN = 0, 2
REPORT_MAX = 64


@pytest.fixture(scope="module")
def pool_key(tmp_path_factory):
    """The (130, 2, 1) mixed circuit with its set-up key, its .r1cs file, the good witness (twice) and two that break different
    constraints; and the .r1cs file of another circuit of the same size."""
    import k16
    from test_boundary import ROOT, PKG
    tmp = tmp_path_factory.mktemp("pool_checked")
    circuit, w = sr.mixed(130, 2, 1)
    n_wires, rowsA, rowsB, rowsC, n_pub_out, n_pub_in = circuit
    n_public = n_pub_out + n_pub_in
    raw = rb.write(n_wires, rowsA, rowsB, rowsC, n_pub_out=n_pub_out, n_pub_in=n_pub_in)
    ctx = k16.Context(0)
    try:
        circ = k16.R1cs(ctx, raw)
        zkey = circ.setup(sr.TRAPDOOR)
        circ.close()
    finally:
        ctx.close()
    k = dict(zk=str(tmp / "pool.zkey"), r1cs=str(tmp / "pool.r1cs"), other=str(tmp / "other.r1cs"), rows=(rowsA, rowsB, rowsC))
    open(k["zk"], "wb").write(zkey)
    open(k["r1cs"], "wb").write(raw)
    open(k["other"], "wb").write(rb.write(n_wires, rowsB, rowsA, rowsC, n_pub_out=n_pub_out, n_pub_in=n_pub_in))   # A and B swapped
    broken = []
    for wire in range(n_public + 1, n_wires):                     # two private wires whose change breaks different constraints
        w2 = list(w)
        w2[wire] = (w2[wire] + 1) % R
        want = rb.check(rowsA, rowsB, rowsC, w2)
        if want and all(want != b[1] for b in broken):
            broken.append((w2, want))
        if len(broken) == 2:
            break
    assert len(broken) == 2
    k["wits"] = [(w, NONE, [])] + [(w2, BROKEN, want) for w2, want in broken] + [(w, NONE, [])]
    k["paths"] = []
    for i, (wi, _, _) in enumerate(k["wits"]):
        k["paths"].append(str(tmp / ("w%d.wtns" % i)))
        vkb.write_wtns(k["paths"][-1], rb.witness_bytes(wi))
    exe = str(tmp / "fullprover_checked_harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "fullprover_checked_harness.cpp"),
                           "-L", PKG, "-lk16", "-Wl,-rpath," + PKG, "-pthread", "-o", exe])
    k["exe"] = exe
    return k


def run(k, r1cs, verify, reps=3, log=False):
    env = dict(os.environ, K16_DEVICES="0,0")
    env.pop("K16_LOG", None)
    if log:
        env["K16_LOG"] = "1"
    out = subprocess.run([k["exe"], k["zk"], r1cs, ",".join(k["paths"]), str(int(verify)), str(reps)], capture_output=True,
                         text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout.splitlines(), out.stderr


def calls(lines):
    """[(witness, 'mem' | 'file', outcome, status, n, list)] of the harness's per-call lines"""
    got = []
    for ln in lines:
        if not ln.startswith("t="):
            continue
        f = ln.split()
        kv = dict(x.split("=", 1) for x in f if "=" in x)
        outcome = int(kv["rc"]) if f[1] == "mem" else (int(kv["type"]), int(kv["error"]))
        got.append((int(kv["t"]), f[1], outcome, int(kv["status"]), int(kv["n"]), [int(x) for x in kv["list"].split(",") if x]))
    return got


@pytest.mark.parametrize("verify", [False, True], ids=["check_only", "check_and_verify"])
def test_each_thread_gets_its_own_rejection(pool_key, verify):
    k = pool_key
    lines, err = run(k, k["r1cs"], verify, log=True)
    head = ["state=0", "r1cs=0"] + (["verify=0"] if verify else [])
    assert lines[:len(head)] == head, (lines[:4], err[-2000:])
    got = calls(lines)
    assert len(got) == 4 * 3 * 2
    for t, how, outcome, status, n, lst in got:
        _, want_status, want = k["wits"][t]
        assert (status, n, lst) == (want_status, len(want), want[:REPORT_MAX]), (t, how)
        if how == "mem":
            assert outcome == (0 if want_status == NONE else ERR_FORMAT), (t, outcome)
        else:
            assert outcome == ((0, 0) if want_status == NONE else (1, 2)), (t, outcome)      # SUCCESS / ERROR, INVALID_INPUT
    assert lines[-1] == "idle status=0 n=0 list="
    # K16_LOG=1: one line per rejected prove, with the count and the list
    logged = [ln for ln in lines if "R1CS check" in ln]
    assert len(logged) == 2 * 3 * 2
    want = k["wits"][1][2]
    assert sum(("%d broken constraints, lowest [%s]" % (len(want), ",".join(map(str, want[:REPORT_MAX])))) in ln for ln in logged) == 3 * 2


def test_circuit_of_another_key_is_refused_and_the_provers_work_unchecked(pool_key):
    k = pool_key
    lines, err = run(k, k["other"], False, reps=1)
    assert lines[:2] == ["state=0", "r1cs=%d" % ERR_FORMAT], (lines[:3], err[-2000:])
    assert "is not the circuit of" in err and "mismatch" in err
    got = calls(lines)
    assert len(got) == 4 * 2
    for t, how, outcome, status, n, lst in got:
        assert (status, n, lst) == (NONE, 0, []), (t, how)
        assert outcome == (0 if how == "mem" else (0, 0)), (t, how, outcome)  # a proof, for the broken witnesses too
