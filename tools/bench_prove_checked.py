"""Checked proving (k16_prover_set_r1cs: the R1CS check rides on the proof) against the two-call way and against a prover with
nothing attached, in fresh processes, alternating call by call.
    python tools/bench_prove_checked.py [--rounds 5] [--proofs 60] [--warmup 10] [--scale 1.0] [--parent-pkg DIR] [--out FILE.json]
Key: the valid SYNTHETIC key of the Keyless shape (tests/valid_key_builder.py: nVars 1,343,588, N = 2^21, one public input)
and its circuit as an .r1cs file (tests/r1cs_builder.py); rows of 1-2 terms, so the timings are the synthetic key's.  Legs:
    a  k16_prover_prove_mem_verified, nothing attached
    b  the same call with the circuit attached (k16_prover_set_r1cs); k16_prover_last_check is asserted outside the timed region
    c  a, then k16_r1cs_check_prover_witness: the two calls are timed and added
A round starts one fresh process per variant, one after the other:
    abc     legs a, b, c alternating call by call on one prover (attach / detach outside the timed region)
    plain   leg a alone in a process that never attaches a circuit: no stream, no buffer of the feature exists in it
    parent  leg a alone with k16.py and libk16.so from --parent-pkg (a build of the parent commit), when given
p50 / p99 per leg and process go to --out (default profiles/prove_checked/bench_prove_checked.json).  Shown there:
b below c in how many rounds; b - a; a of `plain` beside a of `parent` with the spread of both over the rounds."""
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


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def pct(xs, q):
    s = sorted(xs)
    return s[min(len(s) - 1, int(round(q * (len(s) - 1))))]


def child(args):
    """one process: its legs, alternating; prints one JSON line"""
    pkg = os.path.abspath(args.pkg)
    if pkg != PKG:
        os.environ["K16_LIB_PATH"] = os.path.join(pkg, "libk16.so")
    sys.path.insert(0, pkg)
    import k16
    d = args.child
    meta = json.load(open(os.path.join(d, "meta.json")))
    wtns = np.load(os.path.join(d, "wtns.npy"))
    wtns = [np.ascontiguousarray(wtns[i]) for i in range(len(wtns))]
    n_vars = meta["n_vars"]
    ctx = k16.Context(0)
    L = ctx.L
    prover = k16.Prover(ctx, os.path.join(d, "key.zkey"))
    V = k16.VerifyingKey.from_zkey(ctx, os.path.join(d, "key.zkey"))
    prover.set_vk(V)
    legs = ["a", "b", "c"] if args.variant == "abc" else ["a"]
    circ = k16.R1cs(ctx, os.path.join(d, "key.r1cs")) if args.variant == "abc" else None
    buf = C.create_string_buffer(4096)
    proof = np.zeros(256, dtype=np.uint8)
    okc, nf = C.c_uint8(0), C.c_uint64(0)
    lst = np.zeros(64, dtype=np.uint32)

    def chk(rc):
        if rc < 0:
            raise k16.K16Error(rc, (L.k16_last_error(ctx.h) or b"").decode())

    def prove(w):
        okc.value = 0
        t0 = time.perf_counter()
        rc = L.k16_prover_prove_mem_verified(prover.h, _p(w), n_vars, None, None, buf, 4096, None, _p(proof), C.byref(okc))
        ms = (time.perf_counter() - t0) * 1e3
        chk(rc)
        return ms

    def leg_a(i):
        ms = prove(wtns[i])
        assert okc.value == 1
        return ms

    def leg_b(i):
        prover.set_r1cs(circ)
        ms = prove(wtns[i])
        assert okc.value == 1 and prover.last_check() == (k16.CHECK_SATISFIED, 0, [])
        prover.set_r1cs(None)
        return ms

    def leg_c(i):
        ms = leg_a(i)
        t0 = time.perf_counter()
        rc = L.k16_r1cs_check_prover_witness(prover.h, circ.h, C.byref(nf), _p(lst), 64)
        ms += (time.perf_counter() - t0) * 1e3
        chk(rc)
        assert nf.value == 0
        return ms

    fn = {"a": leg_a, "b": leg_b, "c": leg_c}
    row = {"variant": args.variant}
    if circ is not None:                                          # the wrong witness: the proof's verdict is the reference checker's
        bad = np.load(os.path.join(d, "bad.npy"))
        prover.set_r1cs(circ)
        prove(bad)
        assert okc.value == 0 and prover.last_check() == (k16.CHECK_BROKEN, len(meta["bad_want"]), meta["bad_want"][:64])
        prover.set_r1cs(None)
        row["wrong_witness_named"] = meta["bad_want"][:64]
    for k in range(args.warmup):
        for leg in legs:
            fn[leg](k % len(wtns))
    t = {leg: [] for leg in legs}
    for k in range(args.proofs):
        for leg in legs:
            t[leg].append(fn[leg](k % len(wtns)))
    for leg in legs:
        row[leg] = {"p50_ms": statistics.median(t[leg]), "p99_ms": pct(t[leg], 0.99), "min_ms": min(t[leg])}
    if circ is not None:                                          # the kernels by HIP events, in a pass of their own
        ctx.stats_enable(True)
        ctx.stats_reset()
        for k in range(20):
            leg_b(k % len(wtns))
        row["kernel_us"] = {}
        for name in ("r1cs_rows", "r1cs_judge", "r1cs_summary"):
            n_l, ms = ctx.stats_get(name)
            row["kernel_us"][name] = {"launches": n_l, "mean_us": ms * 1e3 / max(n_l, 1)}
        ctx.stats_enable(False)
        circ.close()
    print("ROW " + json.dumps(row), flush=True)
    prover.close()
    V.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--proofs", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0, help="shrinks the circuit (rehearsals)")
    ap.add_argument("--parent-pkg", default=None, help="directory with k16.py and libk16.so of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prove_checked", "bench_prove_checked.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--variant", default="abc", help=argparse.SUPPRESS)
    ap.add_argument("--pkg", default=PKG, help=argparse.SUPPRESS)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    if args.child:
        return child(args)
    sys.path.insert(0, PKG)
    import k16
    import r1cs_builder as rb
    import valid_key_builder as vkb

    d = tempfile.mkdtemp(prefix="k16_bench_checked_")
    try:
        ctx = k16.Context(0)
        t0 = time.time()
        key = vkb.build(lambda g, sc: ctx.synth_points_scalars(g, sc), int(1209229 * args.scale), int(107487 * args.scale),
                        int(26870 * args.scale), seed=17)
        with open(os.path.join(d, "key.zkey"), "wb") as f:
            f.write(key["zkey"])
        raw = rb.write_from_shape(key["shape"])
        with open(os.path.join(d, "key.r1cs"), "wb") as f:
            f.write(raw)
        circ = k16.R1cs(ctx, raw)
        assert circ.match_zkey(key["zkey"]) == 0
        key["zkey"] = None
        info = circ.info()
        wtns = np.stack([np.ascontiguousarray(vkb.fast_witness(key["shape"], 100 + i)[0], dtype=np.uint8) for i in range(4)])
        np.save(os.path.join(d, "wtns.npy"), wtns)
        prods = key["shape"]["prods"]
        bad = wtns[0].copy()
        bad[prods[len(prods) // 2][0], 0] ^= 1
        np.save(os.path.join(d, "bad.npy"), bad)
        want = rb.check(*rb.from_shape(key["shape"])[1:4], rb.witness_ints(bad))
        assert want
        # the device footprint of one attached circuit (coefficients, plan, 3 M row sums, mask, witness buffers)
        hip = C.CDLL("libamdhip64.so")
        free0, free1, total = C.c_size_t(), C.c_size_t(), C.c_size_t()
        hip.hipMemGetInfo(C.byref(free0), C.byref(total))
        second = k16.R1cs(ctx, raw)
        hip.hipMemGetInfo(C.byref(free1), C.byref(total))
        second.close()
        circ.close()
        ctx.close()
        json.dump({"n_vars": key["n_vars"], "bad_want": want}, open(os.path.join(d, "meta.json"), "w"))
        print("key, circuit and witnesses ready in %.0f s" % (time.time() - t0), flush=True)
        out = {"gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "n_vars": key["n_vars"], "domain": key["domain"],
               "n_constraints": info["n_constraints"], "n_terms": info["n_terms"], "proofs_per_leg_per_process": args.proofs,
               "warmup_per_leg": args.warmup, "circuit_device_bytes_per_slot": free0.value - free1.value,
               "legs": {"a": "prove_mem_verified, nothing attached", "b": "prove_mem_verified, circuit attached",
                        "c": "a + k16_r1cs_check_prover_witness"},
               "variants": {"abc": "a, b, c alternating in one process", "plain": "a alone, this build, never attached",
                            "parent": "a alone, the parent commit's build"}, "rounds": []}
        variants = ["abc", "plain"] + (["parent"] if args.parent_pkg else [])
        for rnd in range(args.rounds):
            row = {}
            for v in variants:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", d, "--variant", v, "--proofs", str(args.proofs),
                       "--warmup", str(args.warmup), "--pkg", args.parent_pkg if v == "parent" else PKG]
                res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
                lines = [ln for ln in res.stdout.splitlines() if ln.startswith("ROW ")]
                if res.returncode != 0 or not lines:
                    raise RuntimeError("child %s failed (%d): %s" % (v, res.returncode, res.stderr[-2000:]))
                row[v] = json.loads(lines[-1][4:])
            row["b_below_c"] = row["abc"]["b"]["p50_ms"] < row["abc"]["c"]["p50_ms"]
            out["rounds"].append(row)
            print("round %d  " % rnd + "   ".join("%s p50 %.3f p99 %.3f" % (leg, row["abc"][leg]["p50_ms"], row["abc"][leg]["p99_ms"]) for leg in "abc") +
                  "   " + "   ".join("%s a p50 %.3f" % (v, row[v]["a"]["p50_ms"]) for v in variants[1:]), flush=True)
        med = lambda xs: statistics.median(xs)
        p50 = {leg: med([r["abc"][leg]["p50_ms"] for r in out["rounds"]]) for leg in "abc"}
        out["p50_of_rounds_ms"] = p50
        out["p99_max_of_rounds_ms"] = {leg: max(r["abc"][leg]["p99_ms"] for r in out["rounds"]) for leg in "abc"}
        out["b_below_c_rounds"] = sum(r["b_below_c"] for r in out["rounds"])
        out["b_minus_a_ms"] = p50["b"] - p50["a"]
        out["c_minus_a_ms"] = p50["c"] - p50["a"]
        out["unattached_a_p50_ms"] = {v: {"median": med([r[v]["a"]["p50_ms"] for r in out["rounds"]]),
                                          "spread": [min(r[v]["a"]["p50_ms"] for r in out["rounds"]), max(r[v]["a"]["p50_ms"] for r in out["rounds"])]}
                                      for v in variants[1:]}
        out["kernel_us"] = out["rounds"][-1]["abc"].get("kernel_us")
        print(json.dumps({k: v for k, v in out.items() if k != "rounds"}))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
