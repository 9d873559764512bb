"""Folded batch verification (k16_verify_batch_folded) against k16_verify_batch_checked, same process, alternating.
    python tools/bench_verify_fold.py [--sizes 64,256,...] [--reps 20] [--warmup 3] [--out FILE.json]
All-valid batches under a trapdoor key with n_ic = 2 (the Keyless shape: one public input), built on the device
(tests/fold_reference.py).  Both calls are timed around the C entry point on prepared arrays (no Python marshalling in the
window); the calls end in a stream synchronise.  Reported per size: p50 and min-max of each call in ms.  Then, outside the
timed runs: the library's per-stage event statistics of the fold, one row with a single wrong proof (the fallback's cost),
and the per-proof path's time for ONE proof next to the fold's single final exponentiation.
--quick runs a fixed small set once (for a kernel trace under rocprofv3)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "keyless-zk-proofs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import k16  # noqa: E402
import fold_reference as fr  # noqa: E402

STAGES = ["fold_prepare", "fold_reduce", "msm_sort", "msm_accumulate", "msm_reduce", "fold_miller", "fold_product", "fold_finalexp"]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Batch:
    def __init__(self, proofs, inputs):
        self.n = len(proofs)
        self.pr = np.frombuffer(b"".join(proofs), dtype=np.uint8).copy()
        self.inp = np.frombuffer(b"".join(int(x).to_bytes(32, "little") for r in inputs for x in r), dtype=np.uint8).copy()
        self.ok = np.zeros(self.n, dtype=np.uint8)
        self.why = np.zeros(self.n, dtype=np.uint8)


def call_folded(ctx, V, b):
    folded = C.c_uint8(0)
    t0 = time.perf_counter()
    rc = ctx.L.k16_verify_batch_folded(ctx.h, V.h, _p(b.pr), _p(b.inp), b.n, _p(b.ok), _p(b.why), C.byref(folded))
    ms = (time.perf_counter() - t0) * 1e3
    ctx._chk(rc)
    return ms, bool(folded.value)


def call_checked(ctx, V, b):
    t0 = time.perf_counter()
    rc = ctx.L.k16_verify_batch_checked(ctx.h, V.h, _p(b.pr), _p(b.inp), b.n, _p(b.ok), _p(b.why))
    ms = (time.perf_counter() - t0) * 1e3
    ctx._chk(rc)
    return ms


def summary(xs):
    return {"p50_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "reps": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,256,1024,2048,2049,3072,4096,16384,65536")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",")]
    if args.quick:
        sizes, args.reps, args.warmup = [16384], 3, 1
    ctx = k16.Context(0)
    pts = lambda group, scalars: ctx.synth_points_scalars(group, scalars)
    vk, t = fr.build_key(2, seed=7, points=pts)
    V = k16.VerifyingKey(ctx, vk)
    nmax = max(sizes + [16384])
    inputs = [[(i * 0x9E3779B97F4A7C15 + 12345) % (1 << 253)] for i in range(nmax)]
    proofs = fr.make_proofs(t, inputs, seed=8, points=pts)
    out = {"fold_min": k16.VERIFY_FOLD_MIN, "n_ic": 2, "reps": args.reps, "warmup": args.warmup, "sizes": []}
    for n in sizes:
        b = Batch(proofs[:n], inputs[:n])
        # the fold itself also below the threshold: k16_verify_batch_folded forwards there, so the cross-over is measured
        # with the library's own stages through the parity entry point (caller's weights; same device work)
        w = np.frombuffer(os.urandom(16 * n), dtype=np.uint8).copy()
        gt = np.zeros(384, dtype=np.uint8)

        def call_fold_only():
            t0 = time.perf_counter()
            rc = ctx.L.k16_verify_fold_gt(ctx.h, V.h, _p(b.pr), _p(b.inp), b.n, _p(w), _p(gt))
            ms = (time.perf_counter() - t0) * 1e3
            ctx._chk(rc)
            return ms

        tf, tc, tg = [], [], []
        for rep in range(args.warmup + args.reps):
            ms_f, folded = call_folded(ctx, V, b)
            assert b.ok.all() and not b.why.any() and folded == (n >= k16.VERIFY_FOLD_MIN)
            ms_c = call_checked(ctx, V, b)
            assert b.ok.all() and not b.why.any()
            ms_g = call_fold_only()
            assert gt.tobytes() == fr.GT_ONE
            if rep >= args.warmup:
                tf.append(ms_f)
                tc.append(ms_c)
                tg.append(ms_g)
        row = {"n": n, "folded_call": summary(tf), "checked_call": summary(tc), "fold_any_n": summary(tg),
               "folded": n >= k16.VERIFY_FOLD_MIN}
        # per-stage event statistics of the fold, in runs of their own
        ctx.stats_enable(1)
        ctx.stats_reset()
        k = 5
        for _ in range(k):
            call_fold_only()
        row["fold_stage_ms"] = {s: ctx.stats_get(s)[1] / k for s in STAGES}
        ctx.stats_enable(0)
        out["sizes"].append(row)
        print("n=%6d  folded call p50 %8.3f ms [%.3f, %.3f]   checked p50 %8.3f ms [%.3f, %.3f]   fold (any n) p50 %8.3f ms   stages %s"
              % (n, row["folded_call"]["p50_ms"], row["folded_call"]["min_ms"], row["folded_call"]["max_ms"],
                 row["checked_call"]["p50_ms"], row["checked_call"]["min_ms"], row["checked_call"]["max_ms"],
                 row["fold_any_n"]["p50_ms"], " ".join("%s %.3f" % (s[5:] if s.startswith("fold_") else s, v)
                                                         for s, v in row["fold_stage_ms"].items())), flush=True)
    # the fallback: 16384 proofs, one of them wrong
    n = 16384
    bad = list(proofs[:n])
    bad[n // 2] = fr.make_proofs(t, [inputs[n // 2]], seed=99, points=pts, c_shift={0: 1})[0]
    b = Batch(bad, inputs[:n])
    tb = []
    for rep in range(args.warmup + args.reps):
        ms, folded = call_folded(ctx, V, b)
        assert not folded and b.ok.sum() == n - 1 and not b.ok[n // 2] and b.why[n // 2] == 4
        if rep >= args.warmup:
            tb.append(ms)
    out["one_bad_proof_16384"] = summary(tb)
    print("n= 16384 with one wrong proof (fold + per-proof path): p50 %.3f ms [%.3f, %.3f]"
          % (out["one_bad_proof_16384"]["p50_ms"], out["one_bad_proof_16384"]["min_ms"], out["one_bad_proof_16384"]["max_ms"]))
    # ONE proof on the per-proof (wave-cooperative) path, whole call, next to the fold's single final exponentiation
    b1 = Batch(proofs[:1], inputs[:1])
    t1 = []
    for rep in range(args.warmup + args.reps):
        ms = call_checked(ctx, V, b1)
        if rep >= args.warmup:
            t1.append(ms)
    out["checked_call_one_proof"] = summary(t1)
    fe = [r["fold_stage_ms"]["fold_finalexp"] for r in out["sizes"]]
    out["fold_finalexp_ms"] = {"min": min(fe), "max": max(fe)}
    print("one proof, checked call p50 %.3f ms; fold's final exponentiation (event time) %.3f .. %.3f ms"
          % (out["checked_call_one_proof"]["p50_ms"], min(fe), max(fe)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    V.close()
    ctx.close()


if __name__ == "__main__":
    main()
