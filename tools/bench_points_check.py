"""Times the GPU point checks (csrc/points_check.hip): checked against unchecked verification, the G2 subgroup check at
scale, and the check of a whole Keyless-shape proving key.
    python tools/bench_points_check.py [--out profiles/.../points_check.json] [--reps 200] [--legs verify,g2,zkey]
Checked (k16_verify_batch_checked) and unchecked (k16_verify_batch) verification alternate call by call in one process, on
the toy key (the cost of a verification does not depend on the circuit).  Kernel and host-to-device times come from the
library's kernel stats (HIP events around each launch / copy) in a separate pass, so the end-to-end figures are taken
without them."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "keyless-zk-proofs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import k16  # noqa: E402
import groth16_io as gio  # noqa: E402
from test_oracle_prove import KNOWN_RS0  # noqa: E402

KEYLESS_NVARS, KEYLESS_DOMAIN = 1343588, 1 << 21


def p50(xs):
    return float(np.percentile(np.array(xs), 50))


def verify_leg(ctx, reps):
    V = k16.VerifyingKey(ctx, gio.vk_from_json(os.path.join(ROOT, "tests", "golden", "toy", "toy_vk.json")))
    known = gio.proof_from_json(KNOWN_RS0)
    out = []
    for n in (1, 64, 2048, 16384):
        r = reps if n <= 64 else max(10, reps // 10 if n <= 2048 else reps // 20)
        pr, inp = [known] * n, [[2]] * n
        V.verify_batch(pr, inp)                          # warm-up of both entry points at this size
        V.verify_batch_checked(pr, inp)
        t_u, t_c = [], []
        for _ in range(r):
            t0 = time.perf_counter()
            ok_u = V.verify_batch(pr, inp)
            t1 = time.perf_counter()
            ok_c, why = V.verify_batch_checked(pr, inp)
            t2 = time.perf_counter()
            t_u.append((t1 - t0) * 1e3)
            t_c.append((t2 - t1) * 1e3)
        assert all(ok_u) and all(ok_c) and not any(why)
        out.append(dict(n=n, reps=r, unchecked_p50_ms=p50(t_u), checked_p50_ms=p50(t_c),
                        checked_minus_unchecked_ms=p50(t_c) - p50(t_u)))
        print(json.dumps(out[-1]), flush=True)
    V.close()
    return out


def stats(ctx, names):
    return {nm: ctx.stats_get(nm) for nm in names}


def g2_leg(ctx):
    out = []
    for n in (1 << 20, KEYLESS_NVARS):
        d = ctx.synth_points(k16.G2, 0, n)
        pts = d.download(np.uint8, (n, 128)).copy()
        d.free()
        ctx.points_check(k16.G2, pts[:4096])
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            st = ctx.points_check(k16.G2, pts)
            ts.append((time.perf_counter() - t0) * 1e3)
        assert not st.any()
        ctx.stats_reset()
        ctx.stats_enable(True)
        ctx.points_check(k16.G2, pts)
        s = stats(ctx, ["points_check_g2", "points_check_h2d"])
        ctx.stats_enable(False)
        kms = s["points_check_g2"][1]
        out.append(dict(n=n, total_p50_ms=p50(ts), kernel_ms=kms, kernel_launches=s["points_check_g2"][0],
                        h2d_ms=s["points_check_h2d"][1], g2_points_per_s_kernel=n / kms * 1e3 if kms else None))
        print(json.dumps(out[-1]), flush=True)
    return out


def zkey_leg(ctx):
    import bench
    t0 = time.perf_counter()
    zk = bench.synth_zkey_bytes(ctx, k16, KEYLESS_NVARS, 1, KEYLESS_DOMAIN, 1000)
    t_build = time.perf_counter() - t0
    k16.zkey_check(ctx, zk)                               # warm-up
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        r = k16.zkey_check(ctx, zk)
        ts.append((time.perf_counter() - t0) * 1e3)
    assert r["ok"]
    ctx.stats_reset()
    ctx.stats_enable(True)
    k16.zkey_check(ctx, zk)
    s = stats(ctx, ["points_check_g1", "points_check_g2", "points_check_h2d"])
    ctx.stats_enable(False)
    out = dict(bytes=len(zk), build_s=t_build, total_p50_ms=p50(ts), h2d_ms=s["points_check_h2d"][1],
               kernel_g1_ms=s["points_check_g1"][1], kernel_g2_ms=s["points_check_g2"][1])
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default="")
    ap.add_argument("--legs", default="verify,g2,zkey")
    ap.add_argument("--with-prover", action="store_true",
                    help="verify leg with a prover resident in the same context (its lane and chain streams created by one "
                         "proof first): the checked path's own stream then competes with them for the hardware queues")
    args = ap.parse_args()
    ctx = k16.Context(0)
    legs = args.legs.split(",")
    res = {}
    prover = None
    if args.with_prover:
        toy = os.path.join(ROOT, "tests", "golden", "toy")
        prover = k16.Prover(ctx, os.path.join(toy, "toy_1.zkey"))
        prover.prove_file(os.path.join(toy, "toy.wtns"))
        res["with_prover"] = True
    if "verify" in legs:
        res["verify"] = verify_leg(ctx, args.reps)
    if prover is not None:
        prover.close()
    if "g2" in legs:
        res["g2_check"] = g2_leg(ctx)
    if "zkey" in legs:
        res["zkey_check"] = zkey_leg(ctx)
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
