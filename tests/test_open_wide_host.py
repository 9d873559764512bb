"""CPU tests of the wide classes of the open-set solve (include/k16.h k16_r1cs_open_system_ex / k16_r1cs_open_direction_ex,
DESIGN.md section 10i): the big-integer model of the fraction-free elimination (tests/open_wide_reference.py) against
osr.rref -- the proof that cross-multiplication leaves the zero pattern of the reduced row echelon form; it imports nothing of
the product and passes without it, as reference tests do --, the condition on the wide random family the GPU test shares, the
symbols and constants, and keyless-zk-proofs_amd/csrc/r1cs_open.h with a cap through tests/cpp/r1cs_open_wide_check.cpp, a
stand-alone program built with -fsanitize=address,undefined and run as a plain subprocess.  tests/golden/open_wide/*.txt are
the outputs of tests/cpp/r1cs_open_check.cpp on the same circuits, built against r1cs_open.h as it was before the builder took
a cap: with the cap at 64 the program's output must be those lines."""
import os
import subprocess

import pytest

import open_system_reference as osr
import open_wide_reference as owr
import pymodel as pm
import r1cs_builder as rb
from open_system_reference import ABSENT, FIXED, FORCED, FREE, SKIPPED, UNDECIDED, R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_and_symbols():
    import k16
    assert k16.OPEN_MAX_WIRES == 64 and k16.OPEN_MAX_WIRES_EX == 256
    hdr = open(os.path.join(ROOT, "include", "k16.h")).read()
    for s in ("k16_r1cs_open_system_ex", "k16_r1cs_open_direction_ex"):
        assert s in k16.SYMBOLS and "int  %s(" % s in hdr
        assert hasattr(k16.load(), s)
    assert "#define K16_OPEN_MAX_WIRES 64" in hdr and "#define K16_OPEN_MAX_WIRES_EX 256" in hdr
    import inspect
    for m in ("open_system", "open_direction", "audit"):
        assert inspect.signature(getattr(k16.R1cs, m)).parameters["max_wires"].default is None
    src = open(os.path.join(ROOT, "keyless-zk-proofs_amd", "csrc", "r1cs_scan.hip")).read()
    assert "OPEN_WIDE_ARENA / ((size_t)W * 9 * W * 4)" in src and "OPEN_WIDE_ARENA = (size_t)144 << 20" in src
    assert (144 << 20) // (256 * 9 * 256 * 4) == owr.ARENA_SLABS_256                   # what the GPU test's circuit is sized by


# ---------------------------------------------------------------- the model against rref
def agree(rows, n_cols, p, what):
    """pivots, FORCED set and, after dividing each row by its pivot value, every entry"""
    want_rows, want_pivots = osr.rref([{c: o % p for c, o in row if o % p} for row in rows], n_cols, p)
    basis, pivots = owr.fraction_free(rows, n_cols, p)
    assert sorted(pivots) == want_pivots, what
    assert all(b[q] for b, q in zip(basis, pivots)), what
    want_forced = {q for row, q in zip(want_rows, want_pivots) if all(j in set(want_pivots) for j in row)}
    assert owr.forced_of(basis, pivots) == want_forced, what
    assert owr.normalised(basis, pivots, p) == dict(zip(want_pivots, want_rows)), what
    return len(pivots), len(want_forced)


def test_model_against_rref_over_f7():
    """4,000 random matrices over F_7: up to 8 columns, rows up to twice the columns, rows that are combinations of earlier rows,
    entries that are 0 mod p in the list"""
    ranks, forced, dependent = 0, 0, 0
    for seed in range(4000):
        rows, n_cols = owr.random_matrix(seed, 7)
        rank, n_forced = agree(rows, n_cols, 7, seed)
        ranks += rank
        forced += n_forced
        dependent += len(rows) > rank
    assert ranks > 8000 and forced > 2000 and dependent > 1000, (ranks, forced, dependent)


def test_model_against_rref_over_r():
    """over r: random dense and sparse matrices, and rows that are dependent only mod r (coefficients r - 1)"""
    rng = pm.SplitMix64(0x0F1DE)
    for n_cols, n_rows, width in ((6, 9, 6), (24, 30, 3), (40, 25, 40), (64, 70, 4)):
        rows = []
        for k in range(n_rows):
            cols = sorted({(k + j) % n_cols for j in range(width)} | {rng.next() % n_cols})
            rows.append([(c, 1 + rng.below(R - 1)) for c in cols])
        agree(rows, n_cols, R, (n_cols, n_rows))
    a, b = [1, 2, 3, R - 1], [R - 1, 5, R - 2, 7]
    rows = [list(enumerate(a)), list(enumerate(b))]
    for _ in range(6):                                                     # combinations that cancel only mod r
        k0, k1 = rng.below(R), R - 1 - rng.next() % 3
        rows.append([(j, (k0 * a[j] + k1 * b[j]) % R) for j in range(4)])
    basis, pivots = owr.fraction_free(rows, 4, R)
    assert agree(rows, 4, R, "mod r")[0] == 2 and pivots == [0, 1]
    rows = [[(0, R - 1), (1, 2)], [(0, (R - 1) * (R - 1) % R), (1, 2 * (R - 1) % R)]]     # osr's 2x2_singular_mod_r
    assert agree(rows, 2, R, "2x2")[0] == 1


def test_model_on_the_wide_circuits():
    """the model on the J of every component of two circuits the GPU test runs"""
    for res in (owr.result("redundant_100"), owr.wide_random_result(0)):
        for k in res["comps"].values():
            col = {s: j for j, s in enumerate(k["wires"])}
            rows = [[(col[s], v) for s, v in sorted(res["lin_rows"][i].items())] for i in k["rows"]]
            basis, pivots = owr.fraction_free(rows, len(col), R)
            assert sorted(pivots) == k["pivots"]
            assert owr.normalised(basis, pivots, R) == dict(zip(k["pivots"], k["R"]))


# ---------------------------------------------------------------- the circuits the GPU test shares
def test_wide_circuits_are_what_they_claim():
    for n in owr.CHAIN_SIZES:
        assert owr.result("chain_%d_anchored" % n)["classes"] == [FIXED] + [FORCED] * n
        res = owr.result("chain_%d_open" % n)
        assert res["classes"] == [FIXED] + [FREE] * n and res["comps"][1]["rank"] == n - 1
    assert owr.result("chain_257_open")["classes"] == [FIXED] + [SKIPPED] * 257
    assert owr.result("chain_129_open", 128)["n_skipped"] == 129 and owr.result("chain_129_open")["n_free"] == 129
    res = owr.result("dense_128_full")
    assert res["comps"][1]["rank"] == 128 and res["n_forced"] == 128
    res = owr.result("dense_128_100")
    assert res["n_free"] == 128 and res["n_dims"] == 28
    assert owr.result("dense_256_40")["n_dims"] == 216 and owr.result("dense_200_full")["n_forced"] == 200
    res = owr.result("redundant_100")
    assert res["comps"][1]["rank"] == 2 and len(res["comps"][1]["rows"]) == 12 and res["n_free"] == 100
    res = owr.result("cross_chain")
    assert res["classes"] == [FIXED] + [FORCED] * 100 + [UNDECIDED] and res["n_components"] == 1
    assert osr.analyse(**owr.circuit("cross_chain"))["n_skipped"] == 101
    res = owr.result("chain_130_broken")
    assert res["classes"] == [FIXED] + [FREE] * 130 and res["comps"][1]["rank"] == 129 and len(res["broken"]) == 1


def test_wide_random_family_condition():
    """what the family the GPU test shares must hold, from the reference alone"""
    count = {FORCED: 0, FREE: 0, UNDECIDED: 0, SKIPPED: 0}
    rich, cross_forced = {128: 0, 256: 0}, {128: 0, 256: 0}
    for seed in range(owr.N_WIDE_RANDOM):
        res = owr.wide_random_result(seed)
        for k in count:
            count[k] += res["classes"].count(k)
        for comp in res["comps"].values():
            n = len(comp["wires"])
            if n <= 64:
                continue
            cls = 128 if n <= 128 else 256
            rich[cls] += comp["exact"] and comp["rank"] >= 2 and n - comp["rank"] >= 1
            cross_forced[cls] += comp["cross"] > 0 and any(res["classes"][s] == FORCED for s in comp["wires"])
    assert count[SKIPPED] == 0 and min(count[FORCED], count[FREE], count[UNDECIDED]) >= 10, count
    assert min(rich.values()) >= 3 and min(cross_forced.values()) >= 1, (rich, cross_forced)


# ---------------------------------------------------------------- r1cs_open.h with a cap
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("open_wide_host") / "r1cs_open_wide_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "keyless-zk-proofs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "r1cs_open_wide_check.cpp"), "-o", out], timeout=600)
    return out


def run(exe, path, c, res, cap, wire=None):
    args = [exe, path, ",".join(map(str, c["fixed"])) or "-", ",".join(map(str, res["broken"])) or "-", str(cap)]
    out = subprocess.run(args + ([str(wire)] if wire is not None else []), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and not out.stderr and "FAIL" not in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout.splitlines()


def parse_components(lines):
    """[(id, cross, wires, [(constraint, [(column, wire)])])] in the program's order"""
    comps = []
    for ln in lines:
        f = ln.split()
        if f[0] == "component":
            comps.append((int(f[1]), int(f[2].split("=")[1]), [int(x) for x in f[3].split("=")[1].split(",")], []))
        elif f[0] == "row":
            comps[-1][3].append((int(f[1]), [tuple(int(x) for x in e.split(":")) for e in f[2:]]))
    return comps


def expected_component(res, cid):
    k = res["comps"][cid]
    rows = [(i, [(k["wires"].index(s), s) for s in sorted(res["lin_rows"][i])]) for i in k["rows"]]
    return (cid, k["cross"], k["wires"], rows)


def size_class(n):
    return sum(n > edge for edge in (16, 32, 64, 128))


def mixed_circuit():
    """chains of every class side by side, some anchored, some with a product row, and two components above every cap"""
    sizes = [3, 257, 64, 65, 17, 128, 129, 300, 256, 33, 100]
    return owr.chains_side_by_side(sizes, 71, lambda i: i % 3 != 1, lambda i: i % 4 == 2)


HOST_CASES = [("chain_%d" % n, lambda n=n: osr.chain(n, n % 2 == 0)) for n in (64, 65, 128, 129, 256, 257)] + \
             [("mixed", mixed_circuit), ("wide_random_2", lambda: owr.wide_random_case(2))]


@pytest.mark.parametrize("cap", [64, 128, 256, 100])
def test_host_program(exe, tmp_path, cap):
    for name, make in HOST_CASES:
        c = make()
        res = osr.analyse(c["circuit"], c["w"], c["fixed"], max_wires=cap)
        path = str(tmp_path / (name + ".r1cs"))
        with open(path, "wb") as f:
            f.write(rb.write(*c["circuit"]))
        lines = run(exe, path, c, res, cap)
        assert lines[0] == "kinds " + "".join(map(str, res["kinds"])), name
        sizes = [len(k["wires"]) for k in res["comps"].values() if not k["skipped"]]
        assert all(n <= cap for n in sizes) and all(len(k["wires"]) > cap for k in res["comps"].values() if k["skipped"])
        want = "counts components=%d skipped=%d absent=%d classes=%s" % (
            res["n_components"], res["n_skipped"], res["n_absent"], ",".join(str(sum(size_class(n) == k for n in sizes)) for k in range(5)))
        assert lines[1] == want, name
        host_cls = {FIXED: 0, ABSENT: 1, SKIPPED: 5}
        assert lines[2] == "cls " + "".join(str(host_cls.get(k, 2)) for k in res["classes"]), name
        assert lines[3] == "comp " + " ".join("-" if k == osr.NO_COMP else str(k) for k in res["comp"]), name
        live = sorted((cid for cid, k in res["comps"].items() if not k["skipped"]), key=lambda cid: (size_class(len(res["comps"][cid]["wires"])), cid))
        assert parse_components(lines[4:]) == [expected_component(res, cid) for cid in live], name
        if cap == 64:                                                      # the work list of the builder before it took a cap, line by line
            golden = open(os.path.join(ROOT, "tests", "golden", "open_wide", name + ".txt")).read().splitlines()
            assert lines[1].endswith(",0,0") and [lines[0], lines[1][:-4]] + lines[2:] == golden, name
        # the walk from one wire finds the same component, under the same cap
        ends = {k["wires"][-1] for k in res["comps"].values()} if name == "mixed" else {1, len(res["classes"]) - 1}
        for wire in sorted({0} | ends):
            one = run(exe, path, c, res, cap, wire)
            k = res["classes"][wire]
            comp = res["comps"].get(res["comp"][wire])
            if k in (FIXED, ABSENT):
                assert one[0] == "one class=%d wires=0 rows=0 cross=0" % k, (name, wire)
                continue
            assert one[0] == "one class=%d wires=%d rows=%d cross=%d" % (
                5 if comp["skipped"] else 2, len(comp["wires"]), len(comp["rows"]), comp["cross"]), (name, wire)
            assert parse_components(one[1:]) == ([] if comp["skipped"] else [expected_component(res, res["comp"][wire])]), (name, wire)
