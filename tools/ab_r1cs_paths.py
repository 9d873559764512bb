"""Paths a change must not move, a build of the parent commit against this tree on one box.
    python tools/ab_r1cs_paths.py --parent-pkg DIR --out FILE.json [--rounds 5]
DIR holds k16.py and libk16.so of the parent commit.  Per round and side one fresh process each for
    check    the legs of tools/bench_r1cs_check.py: prove_mem_verified, k16_r1cs_check_mem, k16_r1cs_check_prover_witness,
             and behind them the diagnostics of the sums, k16_r1cs_unbound_wires, k16_r1cs_second_values (cap 64) and
             k16_r1cs_determined_wires (the default seed, cap 64, no maps), alternating call by call, 50 calls per leg
    checked  the child mode of tools/bench_prove_checked.py (legs a, b, c: prove_mem_verified unattached, with the circuit
             attached, and followed by the stand-alone check), 60 proofs per leg
on the synthetic key of the Keyless shape those tools use, built once; the sides alternate.  Per leg: the p50 of the round
p50s and their spread per side, and whether this tree's p50 lies within the spread of the parent's own rounds."""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "keyless-zk-proofs_amd")
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def check_child(d, pkg, calls=50, warmup=5):
    if os.path.abspath(pkg) != PKG:
        os.environ["K16_LIB_PATH"] = os.path.join(pkg, "libk16.so")
    sys.path.insert(0, pkg)
    import k16
    meta = json.load(open(os.path.join(d, "meta.json")))
    wtns = np.load(os.path.join(d, "wtns.npy"))
    wtns = [np.ascontiguousarray(wtns[i]) for i in range(len(wtns))]
    n_vars = meta["n_vars"]
    ctx = k16.Context(0)
    L = ctx.L
    prover = k16.Prover(ctx, os.path.join(d, "key.zkey"))
    V = k16.VerifyingKey.from_zkey(ctx, os.path.join(d, "key.zkey"))
    prover.set_vk(V)
    circ = k16.R1cs(ctx, os.path.join(d, "key.r1cs"))
    buf = C.create_string_buffer(4096)
    proof = np.zeros(256, dtype=np.uint8)
    okc, nf = C.c_uint8(0), C.c_uint64(0)
    lst = np.zeros(64, dtype=np.uint32)

    def leg_prove(i):
        t = time.perf_counter()
        rc = L.k16_prover_prove_mem_verified(prover.h, _p(wtns[i]), n_vars, None, None, buf, 4096, None, _p(proof), C.byref(okc))
        ms = (time.perf_counter() - t) * 1e3
        assert rc >= 0 and okc.value == 1
        return ms

    def leg_mem(i):
        t = time.perf_counter()
        rc = L.k16_r1cs_check_mem(ctx.h, circ.h, _p(wtns[i]), n_vars, C.byref(nf), _p(lst), 64)
        ms = (time.perf_counter() - t) * 1e3
        assert rc == 0 and nf.value == 0
        return ms

    def leg_prover(i):
        t = time.perf_counter()
        rc = L.k16_r1cs_check_prover_witness(prover.h, circ.h, C.byref(nf), _p(lst), 64)
        ms = (time.perf_counter() - t) * 1e3
        assert rc == 0 and nf.value == 0
        return ms

    na, nu, n2 = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    free_w, free_c = np.zeros(64, dtype=np.uint32), np.zeros(64, dtype=np.uint8)
    shifts = np.zeros((64, 32), dtype=np.uint8)

    def leg_unbound(i):
        t = time.perf_counter()
        rc = L.k16_r1cs_unbound_wires(circ.h, C.byref(na), C.byref(nu), _p(free_w), _p(free_c), 64, None)
        ms = (time.perf_counter() - t) * 1e3
        assert rc == 0
        return ms

    def leg_second(i):
        t = time.perf_counter()
        rc = L.k16_r1cs_second_values(circ.h, C.byref(n2), _p(free_w), _p(shifts), 64, None)
        ms = (time.perf_counter() - t) * 1e3
        assert rc == 0 and n2.value > 0
        return ms

    nd, nab, no, nr = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)

    def leg_closure(i):
        t = time.perf_counter()
        rc = L.k16_r1cs_determined_wires(circ.h, None, 0, C.byref(nd), C.byref(nab), C.byref(no), C.byref(nr), _p(free_w), 64, None, None, None)
        ms = (time.perf_counter() - t) * 1e3
        assert rc == 0
        return ms

    legs = [("prove", leg_prove), ("mem", leg_mem), ("prover", leg_prover), ("unbound", leg_unbound), ("second", leg_second),
            ("closure", leg_closure)]
    for k in range(warmup):
        for _, fn in legs:
            fn(k % len(wtns))
    t = {name: [] for name, _ in legs}
    for k in range(calls):
        for name, fn in legs:
            t[name].append(fn(k % len(wtns)))
    print("ROW " + json.dumps({name: {"p50_ms": statistics.median(t[name]), "min_ms": min(t[name])} for name, _ in legs}), flush=True)
    circ.close()
    prover.close()
    V.close()
    ctx.close()


def run(cmd):
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("ROW ")]
    if res.returncode != 0 or not lines:
        raise SystemExit("child failed (%d): %s" % (res.returncode, res.stderr[-3000:]))   # nothing more runs after a failure
    return json.loads(lines[-1][4:])


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--check-child":
        return check_child(sys.argv[2], sys.argv[3])
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-pkg", required=True, help="directory with k16.py and libk16.so of the parent commit")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    parent = os.path.abspath(args.parent_pkg)
    sys.path.insert(0, PKG)
    import k16
    import r1cs_builder as rb
    import valid_key_builder as vkb
    d = tempfile.mkdtemp(prefix="k16_unchanged_")
    try:
        t0 = time.time()
        ctx = k16.Context(0)
        key = vkb.build(lambda g, sc: ctx.synth_points_scalars(g, sc), 1209229, 107487, 26870, seed=17)
        open(os.path.join(d, "key.zkey"), "wb").write(key["zkey"])
        key["zkey"] = None
        open(os.path.join(d, "key.r1cs"), "wb").write(rb.write_from_shape(key["shape"]))
        wtns = np.stack([np.ascontiguousarray(vkb.fast_witness(key["shape"], 100 + i)[0], dtype=np.uint8) for i in range(4)])
        np.save(os.path.join(d, "wtns.npy"), wtns)
        prods = key["shape"]["prods"]
        bad = wtns[0].copy()
        bad[prods[len(prods) // 2][0], 0] ^= 1
        np.save(os.path.join(d, "bad.npy"), bad)
        want = rb.check(*rb.from_shape(key["shape"])[1:4], rb.witness_ints(bad))
        assert want
        ctx.close()
        json.dump({"n_vars": key["n_vars"], "bad_want": want}, open(os.path.join(d, "meta.json"), "w"))
        print("key, circuit and witnesses ready in %.0f s" % (time.time() - t0), flush=True)
        rounds = []
        for rnd in range(args.rounds):
            row = {}
            for side, pkg in (("parent", parent), ("tree", PKG)):
                row[side] = {
                    "check": run([sys.executable, os.path.abspath(__file__), "--check-child", d, pkg]),
                    "checked": run([sys.executable, os.path.join(ROOT, "tools", "bench_prove_checked.py"), "--child", d, "--variant", "abc",
                                    "--proofs", "60", "--warmup", "10", "--pkg", pkg]),
                }
            rounds.append(row)
            print("round %d  " % rnd + "   ".join(
                "%s: check prover %.4f mem %.4f unbound %.4f second %.4f closure %.4f  prove a %.3f b(attached) %.3f c %.3f" % (
                    side, row[side]["check"]["prover"]["p50_ms"], row[side]["check"]["mem"]["p50_ms"],
                    row[side]["check"]["unbound"]["p50_ms"], row[side]["check"]["second"]["p50_ms"], row[side]["check"]["closure"]["p50_ms"],
                    row[side]["checked"]["a"]["p50_ms"], row[side]["checked"]["b"]["p50_ms"], row[side]["checked"]["c"]["p50_ms"])
                for side in ("parent", "tree")), flush=True)
        summ = {}
        for side in ("parent", "tree"):
            summ[side] = {}
            for what, grp, leg in (("check_prover_witness", "check", "prover"), ("check_mem", "check", "mem"),
                                   ("unbound_wires", "check", "unbound"), ("second_values", "check", "second"), ("determined_wires", "check", "closure"),
                                   ("prove_verified_unattached", "checked", "a"), ("prove_verified_attached", "checked", "b")):
                xs = [r[side][grp][leg]["p50_ms"] for r in rounds]
                summ[side][what] = {"p50_of_rounds_ms": statistics.median(xs), "spread_ms": [min(xs), max(xs)]}
        for what in summ["tree"]:
            lo, hi = summ["parent"][what]["spread_ms"]
            summ["tree"][what]["within_parent_spread"] = lo <= summ["tree"][what]["p50_of_rounds_ms"] <= hi
        print(json.dumps(summ, indent=1), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"rounds": rounds, "summary": summ}, f, indent=1)
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
