"""The set-up from a trapdoor (k16_r1cs_setup, k16_generator_mul), measured.
    python tools/bench_setup.py [--runs 5] [--reps 3] [--scale 1.0] [--no-ab] [--no-keyless] [--out FILE.json]
Two parts, both into --out (default profiles/setup/bench_setup.json):
  ab       k16_generator_mul against k16_synth_points_scalars, the per-point double-and-add kernel it replaces in the set-up:
           the same 2^20 random 256-bit scalars for G1 and 2^18 for G2, --runs alternating runs of --reps calls each, every
           call timed around its C entry point and a device synchronise of its own; p50 per run and kernel.  The outputs of
           the two kernels are compared byte by byte once.  "wins" = the new kernel's p50 is below the old one's in EVERY run.
  keyless  the full set-up at the Keyless shape: the circuit of tests/valid_key_builder.py as tools/config4_wave.py sizes it
           (1,343,588 wires, 1,236,099 constraints, N = 2^21), written as an .r1cs by r1cs_builder.write_from_shape.  Wall time
           of k16_r1cs_create and of k16_r1cs_setup (second of two calls: the generator tables exist), the stage split from the
           HIP-event pairs of k16_kernel_stats_* (setup_lagrange, setup_columns, setup_points_g1, setup_points_g2; the point
           stages include their copies to the host), and -- for comparison -- the wall time of valid_key_builder.build with
           k16_synth_points_scalars, the only way to such a key before.  The key is then proved with and the proof verified.
The synthetic circuit's rows hold 1-2 terms; the real Keyless circuit has longer rows, so the column stage's time is this
circuit's."""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="shrinks the Keyless circuit (rehearsals)")
    ap.add_argument("--no-ab", action="store_true")
    ap.add_argument("--no-keyless", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "setup", "bench_setup.json"))
    args = ap.parse_args()
    import k16
    import pymodel as pm
    import r1cs_builder as rb
    import valid_key_builder as vkb

    ctx = k16.Context(0)
    L = ctx.L
    result = {"bench": "set-up from a trapdoor", "runs": args.runs, "reps": args.reps}

    if not args.no_ab:
        result["ab"] = {}
        for group, name, n in ((k16.G1, "g1", 1 << 20), (k16.G2, "g2", 1 << 18)):
            w, n_windows = k16.generator_mul_info(group)
            scalars = np.random.RandomState(7 + group).randint(0, 256, size=(n, 32), dtype=np.uint8)
            d_s = ctx.to_device(scalars)
            d_new, d_old = ctx.alloc(n * k16.AFF_BYTES[group]), ctx.alloc(n * k16.AFF_BYTES[group])

            def timed(call, d_out):
                t0 = time.perf_counter()
                ctx._chk(call(ctx.h, group, d_s.ptr, n, d_out.ptr))
                ctx.sync()
                return (time.perf_counter() - t0) * 1e3

            timed(L.k16_generator_mul, d_new)                     # builds the table, sizes the scratch area
            timed(L.k16_synth_points_scalars, d_old)
            same = bool(np.array_equal(d_new.download(), d_old.download()))
            runs = []
            for _ in range(args.runs):
                new = [timed(L.k16_generator_mul, d_new) for _ in range(args.reps)]
                old = [timed(L.k16_synth_points_scalars, d_old) for _ in range(args.reps)]
                runs.append({"generator_mul_p50_ms": round(statistics.median(new), 3),
                             "synth_points_scalars_p50_ms": round(statistics.median(old), 3)})
            result["ab"][name] = {"n": n, "window_bits": w, "n_windows": n_windows, "outputs_equal": same, "runs": runs,
                                  "wins": all(r["generator_mul_p50_ms"] < r["synth_points_scalars_p50_ms"] for r in runs)}
            print(name, json.dumps(result["ab"][name]), flush=True)
            assert same
            for d in (d_s, d_new, d_old):
                d.free()

    if not args.no_keyless:
        sizes = (int(1209229 * args.scale), int(107487 * args.scale), int(26870 * args.scale))
        t0 = time.time()
        key = vkb.build(lambda g, sc: ctx.synth_points_scalars(g, sc), *sizes, seed=11)
        builder_s = time.time() - t0
        shape, n_builder = key["shape"], len(key["zkey"])
        key["zkey"] = None
        t0 = time.time()
        raw = rb.write_from_shape(shape)
        write_s = time.time() - t0
        t0 = time.time()
        circ = k16.R1cs(ctx, raw)
        create_s = time.time() - t0
        rng = pm.SplitMix64(2024)
        trapdoor = [1 + rng.below(pm.R - 1) for _ in range(5)]
        t0 = time.time()
        zkey = circ.setup(trapdoor)                               # first call: builds both generator tables
        first_s = time.time() - t0
        ctx.stats_enable(True)
        ctx.stats_reset()
        t0 = time.time()
        zkey = circ.setup(trapdoor)
        setup_s = time.time() - t0
        stages = {}
        for name in ("setup_lagrange", "setup_columns", "setup_points_g1", "setup_points_g2"):
            launches, ms = ctx.stats_get(name)
            stages[name] = {"launches": launches, "ms": round(ms, 2)}
        ctx.stats_enable(False)
        assert circ.match_zkey(zkey) == 0
        info = circ.info()
        # the key's purpose: a proof made with it verifies
        tmp = tempfile.mkdtemp(prefix="k16_setup_")
        zk = os.path.join(tmp, "key.zkey")
        with open(zk, "wb") as f:
            f.write(zkey)
        prover, V = k16.Prover(ctx, zk), k16.VerifyingKey.from_zkey(ctx, zk)
        os.remove(zk)
        os.rmdir(tmp)
        prover.set_vk(V)
        wb, pub = vkb.fast_witness(shape, 100)
        js, proof, ok = prover.prove_mem_verified(wb)
        wb[shape["prods"][5][0], 0] ^= 1
        js, proof, bad_ok = prover.prove_mem_verified(wb)
        prover.close()
        V.close()
        circ.close()
        result["keyless"] = {
            "n_wires": info["n_wires"], "n_constraints": info["n_constraints"], "n_terms": info["n_terms"],
            "domain": key["domain"], "zkey_bytes": len(zkey), "builder_zkey_bytes": n_builder,
            "g1_points": 3 * info["n_wires"] + key["domain"], "g2_points": info["n_wires"],
            "r1cs_write_python_s": round(write_s, 2), "r1cs_create_s": round(create_s, 3),
            "setup_first_call_s": round(first_s, 3), "setup_s": round(setup_s, 3), "stages": stages,
            "setup_host_and_copies_s": round(setup_s - sum(s["ms"] for s in stages.values()) / 1e3, 3),
            "valid_key_builder_with_synth_points_scalars_s": round(builder_s, 2),
            "proof_with_the_key_verifies": int(ok), "proof_of_a_broken_witness_verifies": int(bad_ok)}
        print("keyless", json.dumps(result["keyless"]), flush=True)
        assert ok == 1 and bad_ok == 0
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
