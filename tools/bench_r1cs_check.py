"""The R1CS witness check (k16_r1cs_check_mem, k16_r1cs_check_prover_witness) beside the verified prove whose rejection it
explains, same process, alternating call by call.
    python tools/bench_r1cs_check.py [--runs 8] [--calls 50] [--warmup 5] [--scale 1.0] [--out FILE.json]
Key: the valid SYNTHETIC key of the Keyless shape that tools/config4_wave.py builds (tests/valid_key_builder.py: nVars
1,343,588, 1,236,099 constraints, N = 2^21, one public input); its circuit as an .r1cs file from the builder's `shape`
(tests/r1cs_builder.py).  Its rows hold 1-2 terms (3.7 M terms in all): the real Keyless circuit has 1,376,867 constraints
and longer rows, so these timings are the synthetic key's, not the real circuit's.  Legs:
    prove    k16_prover_prove_mem_verified          -- what a rejected proof has cost by the time it is rejected
    mem      k16_r1cs_check_mem                     -- uploads the 43 MB witness, then checks
    prover   k16_r1cs_check_prover_witness          -- the witness of the prove just before it, read in place
Every call is timed around its C entry point and ends in a device synchronise of its own.  The legs alternate call by call;
p50 and p99 per leg and run go to --out (default profiles/r1cs_check/bench_r1cs_check.json), with the HIP-event times of the
row kernel and the judge kernel from a pass of their own (k16_kernel_stats_*).  Every verdict is asserted: the satisfying
witnesses break nothing, a witness with one product wire changed breaks what the reference checker names."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "keyless-zk-proofs_amd")):
    sys.path.insert(0, p)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def pct(xs, q):
    s = sorted(xs)
    return s[min(len(s) - 1, int(round(q * (len(s) - 1))))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="shrinks the circuit (rehearsals)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r1cs_check", "bench_r1cs_check.json"))
    args = ap.parse_args()
    import k16
    import r1cs_builder as rb
    import valid_key_builder as vkb

    ctx = k16.Context(0)
    L = ctx.L
    t0 = time.time()
    key = vkb.build(lambda g, sc: ctx.synth_points_scalars(g, sc), int(1209229 * args.scale), int(107487 * args.scale),
                    int(26870 * args.scale), seed=17)
    print("key built in %.0f s" % (time.time() - t0), flush=True)
    tmp = tempfile.mkdtemp(prefix="k16_bench_")
    zk = os.path.join(tmp, "key.zkey")
    with open(zk, "wb") as f:
        f.write(key["zkey"])
    prover = k16.Prover(ctx, zk)
    V = k16.VerifyingKey.from_zkey(ctx, zk)
    prover.set_vk(V)
    os.remove(zk)
    os.rmdir(tmp)
    circ = k16.R1cs(ctx, rb.write_from_shape(key["shape"]))
    assert circ.match_zkey(key["zkey"]) == 0
    key["zkey"] = None
    info = circ.info()
    wtns = [np.ascontiguousarray(vkb.fast_witness(key["shape"], 100 + i)[0], dtype=np.uint8) for i in range(4)]
    n_vars = key["n_vars"]
    # one wrong witness, its verdict against the reference checker (not timed)
    c_bad = key["shape"]["prods"][len(key["shape"]["prods"]) // 2][0]
    bad = wtns[0].copy()
    bad[c_bad, 0] ^= 1
    want = rb.check(*rb.from_shape(key["shape"])[1:4], rb.witness_ints(bad))
    n, idx = circ.check(bad)
    assert want and n == len(want) and idx.tolist() == want
    buf = C.create_string_buffer(4096)
    proof = np.zeros(256, dtype=np.uint8)
    okc = C.c_uint8(0)
    nf = C.c_uint64(0)
    lst = np.zeros(64, dtype=np.uint32)

    def chk(rc):
        if rc < 0:
            raise k16.K16Error(rc, (L.k16_last_error(ctx.h) or b"").decode())

    def leg_prove(i):
        t = time.perf_counter()
        rc = L.k16_prover_prove_mem_verified(prover.h, _p(wtns[i]), n_vars, None, None, buf, 4096, None, _p(proof), C.byref(okc))
        ms = (time.perf_counter() - t) * 1e3
        chk(rc)
        assert okc.value == 1
        return ms

    def leg_mem(i):
        t = time.perf_counter()
        rc = L.k16_r1cs_check_mem(ctx.h, circ.h, _p(wtns[i]), n_vars, C.byref(nf), _p(lst), 64)
        ms = (time.perf_counter() - t) * 1e3
        chk(rc)
        assert nf.value == 0
        return ms

    def leg_prover(i):
        t = time.perf_counter()
        rc = L.k16_r1cs_check_prover_witness(prover.h, circ.h, C.byref(nf), _p(lst), 64)
        ms = (time.perf_counter() - t) * 1e3
        chk(rc)
        assert nf.value == 0
        return ms

    legs = [("prove", leg_prove), ("mem", leg_mem), ("prover", leg_prover)]
    for k in range(args.warmup):
        for _, fn in legs:
            fn(k % len(wtns))
    out = {"gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "n_vars": n_vars, "domain": key["domain"],
           "n_constraints": info["n_constraints"], "n_terms": info["n_terms"], "calls_per_leg_per_run": args.calls,
           "warmup_per_leg": args.warmup, "wrong_witness_constraints_named": want,
           "legs": {"prove": "k16_prover_prove_mem_verified", "mem": "k16_r1cs_check_mem", "prover": "k16_r1cs_check_prover_witness"},
           "runs": []}
    for run in range(args.runs):
        t = {name: [] for name, _ in legs}
        for k in range(args.calls):
            for name, fn in legs:
                t[name].append(fn((run + k) % len(wtns)))
        row = {name: {"p50_ms": statistics.median(t[name]), "p99_ms": pct(t[name], 0.99), "min_ms": min(t[name])} for name, _ in legs}
        out["runs"].append(row)
        print("run %d  " % run + "   ".join("%s p50 %.3f p99 %.3f ms" % (name, row[name]["p50_ms"], row[name]["p99_ms"]) for name, _ in legs), flush=True)
    out["p50_of_runs_ms"] = {name: statistics.median(r[name]["p50_ms"] for r in out["runs"]) for name, _ in legs}
    out["p99_max_of_runs_ms"] = {name: max(r[name]["p99_ms"] for r in out["runs"]) for name, _ in legs}
    out["check_over_prove_p50"] = {name: out["p50_of_runs_ms"][name] / out["p50_of_runs_ms"]["prove"] for name in ("mem", "prover")}
    # the two kernels by HIP events, in a pass of their own (the events sit between the launches)
    ctx.stats_enable(True)
    ctx.stats_reset()
    for k in range(args.calls):
        leg_mem(k % len(wtns))
    out["kernel_us"] = {}
    for name in ("r1cs_rows", "r1cs_judge"):
        n_l, ms = ctx.stats_get(name)
        out["kernel_us"][name] = {"launches": n_l, "mean_us": ms * 1e3 / max(n_l, 1)}
    ctx.stats_enable(False)
    print(json.dumps({k: v for k, v in out.items() if k not in ("runs", "wrong_witness_constraints_named")}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    circ.close()
    prover.close()
    V.close()
    ctx.close()


if __name__ == "__main__":
    main()
